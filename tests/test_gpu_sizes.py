"""GPU: training and inference on the large side of the launch code's size switches (tests/size_batches.py), against the suite's
references -- fp64 autograd of the torch graph for gradients (check_grads of test_gpu_training.py), the NumPy oracle for the forward
and its outputs -- and against the same step summed over sub-batches that each sit on the small side of every switch.

Every test first asserts, from the uploaded batch, that it is on the side it is meant to be.  The CPU references are computed once per
module (the 34 k-atom batch's autograd takes tens of seconds)."""
import importlib.util
import os

import numpy as np
import pytest

import scann_oracle as so
import size_batches as sb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_sizes_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tg = _load("test_gpu_training")   # check_grads, grad_reference, grad_errors, OTHER_WIDTHS
tp = _load("test_gpu_parity")     # RTOL, rel_err
to = _load("test_gpu_outputs")    # check_against_oracle, all_names

BATCHES = {"mp2018_b128": sb.mp2018_b128, "qm9_b260": sb.qm9_b260, "sparse_atoms": sb.sparse_atoms}
# gradients whose sums end in float atomics (test_weight_gradients_are_bit_reproducible): the embedding table, the K = 20 basis filters,
# the output head
FLOAT_ATOMIC = ("embed_atom/", "dense_embed/", "neighbor_d/", "neighbor_w/", "predict_property/")


def config(name, widths=None):
    cfg = so.default_config("mp2018" if name.startswith("mp2018") else "qm9")
    cfg["model"]["n_attention"] = 2
    if widths:
        cfg["model"].update(tg.OTHER_WIDTHS[widths])
        cfg["model"]["n_atoms"] = 100  # (setup_widths)
    return cfg, so.init_weights(cfg, 3, perturb=True)


@pytest.fixture(scope="module")
def cache():
    """key -> value, computed on first use for the whole module"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]

    return get


def grad_refs(cache, key, cfg, w, pk, targets, **kw):
    return cache(("grads",) + key, lambda: tg.grad_reference(cfg, w, pk, targets, **kw))


def margin(got, refs, cap=None):
    """worst error / bound over the tensors under check_grads' rule (printed: how much room the step leaves)"""
    _, ref, g32 = refs
    e_gpu, e_32 = tg.grad_errors(got, ref), tg.grad_errors(g32, ref)
    return max(e_gpu[k] / min(cap or tg.GRAD_CAP, max(tg.GRAD_FLOOR, tg.GRAD_SLACK * e_32[k])) for k in ref)


def assert_side(eng, rb, name):
    """the uploaded batch is on the large side of the switches `name` is built to cross (size_batches.LARGE)"""
    info = eng.batch_info(rb)
    assert sb.crosses(name, info["atoms"], info["edges"], info["max_degree"], info["tile_rows"], info["big_atoms"]), (name, info)
    return info


def train_grads(model, pk, targets, name, dropout=0.0, seed=0, begin=True):
    eng = model.engine
    if begin:
        eng.train_begin()
    rb = eng.upload(pk)
    assert_side(eng, rb, name)
    sse = eng.train_forward(rb, targets, dropout=dropout, seed=seed)
    eng.zero_grads()
    eng.train_backward(rb, sse, pk.n_struct)
    got = eng.get_grads()
    rb.free()
    return sse, got


# ---- 1. gradients against fp64 autograd, fused and modular backward ----

@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "modular"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_gradients_at_size_match_autograd(hip_lib, monkeypatch, cache, name, fused):
    """mp2018_b128: edge_bwd_kernel<2, ..>, 64-row edge tiles (unfused attention backward, degree > 16: attn_bwd_kernel), more than four
    wgrad chunks per slab; qm9_b260: attn_bwd16_kernel at 2 atoms per wave; sparse_atoms: rn_bwd_kernel<2>, the KEEP atom_kernel at 64-row
    tiles, 8 atoms per wave, two LayerNorm row groups, wgrad_reduce4_kernel.  SCANN_TRAIN_FUSED=0: ln_bwd_kernel and the modular chain."""
    from scann.models.scann_model import HipModel

    cfg, w = config(name)
    pk, targets = cache(("batch", name), BATCHES[name])
    monkeypatch.setenv("SCANN_TRAIN_FUSED", fused)
    sse, got = train_grads(HipModel(cfg, w, device=0), pk, targets, name)
    refs = grad_refs(cache, (name,), cfg, w, pk, targets)
    rmse, _ = tg.check_grads(got, cfg, w, pk, targets, refs=refs)
    assert abs(np.sqrt(sse / pk.n_struct) - rmse) <= 1e-5 * max(rmse, 1e-6), (np.sqrt(sse / pk.n_struct), rmse)
    print("%s fused=%s: worst gradient error / bound %.3f, rmse rel err %.2e" % (name, fused, margin(got, refs),
                                                                                   abs(np.sqrt(sse / pk.n_struct) - rmse) / rmse))


def test_dropout_gradients_at_size_match_autograd(hip_lib, cache):
    """Attention Dropout (mask element edge * 8 + head: 348 k elements here) and the two Dropout(0.1) layers on the crystal batch"""
    import torch_ref
    from scann.models.scann_model import HipModel

    name, seed, p = "mp2018_b128", 987654321, 0.1
    cfg, w = config(name)
    pk, targets = cache(("batch", name), BATCHES[name])
    model = HipModel(cfg, w, device=0)
    model.engine.train_begin()
    model.engine.set_attention_dropout(p)
    sse, got = train_grads(model, pk, targets, name, dropout=p, seed=seed, begin=False)
    idx = np.arange(pk.n_edge * 8, dtype=np.uint64)
    scales = [torch_ref.drop_scale_np(seed, 2000 + l, idx, p).reshape(pk.n_edge, 8) for l in range(2)]
    assert 0.08 < np.mean(scales[1] == 0) < 0.12
    refs = grad_refs(cache, (name, "drop"), cfg, w, pk, targets, attn_scale=scales, drop=(seed, p))
    rmse, _ = tg.check_grads(got, cfg, w, pk, targets, refs=refs)
    assert abs(np.sqrt(sse / pk.n_struct) - rmse) <= 2e-5 * max(rmse, 1e-6)
    print("%s dropout: worst gradient error / bound %.3f" % (name, margin(got, refs)))


# ---- 2. the same step summed over small sub-batches ----

@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "modular"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_gradients_at_size_equal_the_sum_over_small_sub_batches(hip_lib, monkeypatch, cache, name, fused):
    """train_backward takes the global loss: the gradient of the large batch is the sum of train_backward(sub, sse_total, count_total)
    over sub-batches of it, each small enough for the 32-row / one-atom-per-wave / four-chunk / single-reduce variants.  Only the
    summation order differs, so every gradient whose sums run in a fixed order (per-slab / per-workgroup partial slots: everything the
    size switches partition) is held to the rule of the two-rank RCCL test, 2e-5 of the tensor's rms.  The few tensors that end in
    float atomics (FLOAT_ATOMIC) change their summation order from run to run on either side; at 51 k edges that alone moves the
    heavy-tailed basis-filter gradients by up to ~1.8e-5 of their rms (as far as each side sits from fp64 autograd), so they are held
    to GRAD_FLOOR under grad_errors' normalisation, the measure check_grads applies to every tensor."""
    from scann.models.scann_model import HipModel

    cfg, w = config(name)
    pk, targets = cache(("batch", name), BATCHES[name])
    monkeypatch.setenv("SCANN_TRAIN_FUSED", fused)
    eng = HipModel(cfg, w, device=0).engine
    eng.train_begin()
    check_sum_over_small_sub_batches(eng, pk, targets, lambda rb: assert_side(eng, rb, name), "%s fused=%s" % (name, fused))


def check_sum_over_small_sub_batches(eng, pk, targets, expect, label):
    """the rule of test_gradients_at_size_equal_the_sum_over_small_sub_batches for the training handle `eng` and one batch; `expect(rb)`
    asserts from the uploaded batch that it is on the large side"""
    from scann.parallel import slice_packed

    rb = eng.upload(pk)
    expect(rb)
    sse = eng.train_forward(rb, targets)
    eng.zero_grads()
    eng.train_backward(rb, sse, pk.n_struct)
    g_big = eng.get_grads()
    rb.free()
    cuts = sb.small_cuts(pk)
    subs = []
    for lo, hi in cuts:
        sub = eng.upload(slice_packed(pk, lo, hi))
        info = eng.batch_info(sub)
        assert info["tile_rows"] == 32 and sb.small_side(info["atoms"], info["edges"]), info
        subs.append((sub, targets[lo:hi], hi - lo))
    sse_sub = [eng.train_forward(sub, t) for sub, t, _ in subs]
    sse_tot = float(sum(sse_sub))
    assert abs(sse_tot - sse) <= 1e-5 * sse, (sse_tot, sse)
    eng.zero_grads()
    for (sub, t, _), s in zip(subs, sse_sub):
        assert eng.train_forward(sub, t) == s  # (the sub-batch's kept tensors are this forward's)
        eng.train_backward(sub, sse_tot, pk.n_struct)
    g_sum = eng.get_grads()
    for sub, _, _ in subs:
        sub.free()
    worst = {True: (0.0, ""), False: (0.0, "")}
    atomic_err = tg.grad_errors(g_sum, {k: g_big[k].astype(np.float64) for k in g_big if k.startswith(FLOAT_ATOMIC)})
    for k, ref in g_big.items():
        if k.startswith(FLOAT_ATOMIC):
            err = atomic_err[k]
            assert err <= tg.GRAD_FLOOR, (label, len(cuts), k, err)
        else:
            scale = max(float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))), 1e-12)
            err = float(np.max(np.abs(g_sum[k].astype(np.float64) - ref))) / scale
            assert err <= 2e-5, (label, len(cuts), k, err)
        worst[k.startswith(FLOAT_ATOMIC)] = max(worst[k.startswith(FLOAT_ATOMIC)], (err, k))
    print("%s: %d sub-batches, worst |sum - whole| / rms %.2e (%s; bound 2e-5), float-atomic tensors %.2e (%s; bound %.0e)" % (
        label, len(cuts), worst[False][0], worst[False][1], worst[True][0], worst[True][1], tg.GRAD_FLOOR))
    return len(cuts), worst


# ---- 3. the plain-fp32 training kernels at size ----

def test_plain_fp32_gradients_on_the_sparse_batch(hip_lib, cache):
    """64 / 4 widths on 34 k atoms: gen_layernorm_bwd at more than 64 rows per chunk, gen_dense_dw at 64 slabs"""
    from scann.models.scann_model import HipModel

    name = "sparse_atoms"
    cfg, w = config(name, "64x4")
    pk, targets = cache(("batch", name), BATCHES[name])
    assert pk.n_atom > sb.GEN_LN_64_ROWS_MAX
    sse, got = train_grads(HipModel(cfg, w, device=0), pk, targets, name)
    refs = grad_refs(cache, (name, "64x4"), cfg, w, pk, targets)
    rmse, _ = tg.check_grads(got, cfg, w, pk, targets, refs=refs)
    assert abs(np.sqrt(sse / pk.n_struct) - rmse) <= 2e-5 * max(rmse, 1e-6)
    print("%s 64x4: worst gradient error / bound %.3f" % (name, margin(got, refs)))


def test_plain_fp32_training_cross_checks_the_mfma_path_at_size(hip_lib, monkeypatch, cache):
    """SCANN_GENERIC=1 at 128 / 8 on qm9_b260: the same gradients as the MFMA kernels (rule of
    test_plain_fp32_training_cross_checks_the_mfma_path) and as fp64 autograd"""
    from scann.models.scann_model import HipModel

    name = "qm9_b260"
    cfg, w = config(name)
    pk, targets = cache(("batch", name), BATCHES[name])
    sse_a, ga = train_grads(HipModel(cfg, w, device=0), pk, targets, name)
    monkeypatch.setenv("SCANN_GENERIC", "1")
    plain = HipModel(cfg, w, device=0)
    monkeypatch.delenv("SCANN_GENERIC")
    sse_b, gb = train_grads(plain, pk, targets, name)
    assert abs(sse_a - sse_b) <= 1e-4 * sse_a
    worst = 0.0
    for k in ga:
        scale = max(float(np.abs(ga[k]).max()), 1e-12)
        err = float(np.abs(ga[k] - gb[k]).max()) / scale
        assert err <= 2e-4, (k, err)
        worst = max(worst, err)
    refs = grad_refs(cache, (name,), cfg, w, pk, targets)
    tg.check_grads(gb, cfg, w, pk, targets, refs=refs)
    print("%s plain vs mfma: worst %.2e (bound 2e-4); plain vs autograd: worst error / bound %.3f" % (name, worst, margin(gb, refs)))


# ---- 4. inference at 64-row atom tiles ----

def sparse_oracle(cache, cfg, w):
    def make():
        inputs, _ = sb.padded(sb.sparse_atoms_data())
        y32, ga32 = so.forward(cfg, w, inputs, np.float32)
        y64, ga64 = so.forward(cfg, w, inputs, np.float64)
        return inputs, (y32, ga32), (y64, ga64)

    return cache(("oracle", "sparse_atoms"), make)


def test_inference_on_the_sparse_batch_matches_the_oracle(hip_lib, monkeypatch, cache):
    """atom_kernel<.., 2, ..> in the inference, exact-fp32 (SCANN_EXACT=1) and after_Lc-output families: y and GA scores against the
    oracle at RTOL; the exact kernels to the rule of test_exact_fp32_kernels_match_the_oracle; every layer's attention weights,
    after_Lc and bf_property as test_gpu_outputs.py compares them"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    name = "sparse_atoms"
    cfg, w = config(name)
    pk, _ = cache(("batch", name), BATCHES[name])
    inputs, (y32, ga32), (y64, ga64) = sparse_oracle(cache, cfg, w)
    fast = HipModel(cfg, w, device=0, infer=True)
    rb = fast.engine.upload(pk)
    assert_side(fast.engine, rb, name)
    rb.free()
    y, ga = fast.predict(pk)
    e_y, e_ga = tp.rel_err(y, y32), tp.rel_err(ga, ga32)
    assert e_y <= tp.RTOL and e_ga <= tp.RTOL, (e_y, e_ga)
    monkeypatch.setenv("SCANN_EXACT", "1")
    ex = HipModel(cfg, w, device=0, infer=True)
    monkeypatch.delenv("SCANN_EXACT")
    y_ex, ga_ex = ex.predict(pk)
    b_y, b_ga = max(tp.RTOL, 2 * tp.rel_err(y32, y64)), max(tp.RTOL, 2 * tp.rel_err(ga32, ga64))
    assert tp.rel_err(y_ex, y64) <= b_y and tp.rel_err(ga_ex, ga64) <= b_ga, (tp.rel_err(y_ex, y64), tp.rel_err(ga_ex, ga64))
    assert tp.rel_err(y_ex, y) <= tp.RTOL and tp.rel_err(ga_ex, ga) <= tp.RTOL
    names = to.all_names(cfg)
    packed = fast.predict(pk, outputs=names)
    got = []
    for n, g in zip(names, packed):
        if n.startswith("local_attention_"):
            got.append(_hip.repad_local_attention(g, inputs["atom_mask"], inputs["neighbor_mask"]))
        elif n == "after_Lc":
            got.append(_hip.repad_atoms(g, inputs["atom_mask"]))
        else:
            got.append(g)
    to.check_against_oracle(cfg, w, inputs, got, names)
    print("sparse_atoms inference: y %.2e ga %.2e (bound %.0e); exact: y %.2e (bound %.2e) ga %.2e (bound %.2e)" % (
        e_y, e_ga, tp.RTOL, tp.rel_err(y_ex, y64), b_y, tp.rel_err(ga_ex, ga64), b_ga))


# ---- 5. the largest structure ----

def test_largest_structure_forward_and_gradients(hip_lib, cache):
    """3,000 atoms (the upload limit): readout_kernel with ~60 KB of LDS, readout_bwd_kernel; 3,001 atoms are refused at upload"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    name = "giant"
    cfg, w = config(name)
    pk, targets = sb.giant(sb.UPLOAD_MAX_ATOMS)
    assert int(np.diff(pk.mol_offset).max()) == sb.UPLOAD_MAX_ATOMS
    inputs, _ = sb.padded(sb.giant_data(sb.UPLOAD_MAX_ATOMS))
    model = HipModel(cfg, w, device=0, infer=True)
    y, ga = model.predict(pk)
    y32, ga32 = so.forward(cfg, w, inputs, np.float32)
    e_y, e_ga = tp.rel_err(y, y32), tp.rel_err(ga, ga32)
    assert e_y <= tp.RTOL and e_ga <= tp.RTOL, (e_y, e_ga)
    sums = np.asarray(ga, np.float64).reshape(pk.n_struct, -1).sum(1)
    assert np.max(np.abs(sums - 1.0)) <= 1e-5, sums
    sse, got = train_grads(HipModel(cfg, w, device=0), pk, targets, name)
    refs = grad_refs(cache, ("giant",), cfg, w, pk, targets)
    rmse, _ = tg.check_grads(got, cfg, w, pk, targets, refs=refs)
    assert abs(np.sqrt(sse / pk.n_struct) - rmse) <= 1e-5 * max(rmse, 1e-6)
    print("giant(3000): y %.2e ga %.2e (bound %.0e), |sum ga - 1| %.1e; gradients worst error / bound %.3f" % (
        e_y, e_ga, tp.RTOL, np.max(np.abs(sums - 1.0)), margin(got, refs)))
    pk1, _ = sb.giant(sb.UPLOAD_MAX_ATOMS + 1)
    with pytest.raises(_hip.ScannHipError) as ei:
        model.engine.upload(pk1)
    assert ei.value.code == -2 and "too large" in str(ei.value), str(ei.value)


def test_largest_structure_the_plain_fp32_backward_takes(hip_lib, cache):
    """64 / 4 widths: the GlobalAttention pooling backward holds 3 n + 4 doubles in LDS, so 2,729 atoms train (and match autograd)
    and 2,730 are refused by train_forward -- before the step has touched anything: weights and gradients stay as they were, and an
    ordinary batch trains to the same bits afterwards"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg, w = config("giant", "64x4")
    pk, targets = sb.giant(sb.GEN_BWD_MAX_ATOMS)
    assert int(np.diff(pk.mol_offset).max()) == sb.GEN_BWD_MAX_ATOMS
    sse, got = train_grads(HipModel(cfg, w, device=0), pk, targets, "giant")
    refs = grad_refs(cache, ("giant2729", "64x4"), cfg, w, pk, targets)
    rmse, _ = tg.check_grads(got, cfg, w, pk, targets, refs=refs)
    assert abs(np.sqrt(sse / pk.n_struct) - rmse) <= 2e-5 * max(rmse, 1e-6)
    print("giant(2729) 64x4: gradients worst error / bound %.3f" % margin(got, refs))
    # refused at train_forward
    de, dn = so.synth_dataset(6, 2)
    inputs, t_small = so.pad_batch(de, dn, True)
    small = _hip.pack_inputs(inputs)
    eng = HipModel(cfg, w, device=0).engine
    eng.train_begin()
    rb_small = eng.upload(small)
    s0 = eng.train_forward(rb_small, t_small)
    eng.zero_grads()
    eng.train_backward(rb_small, s0, small.n_struct)
    g0, w0 = eng.get_grads(), eng.get_weights()
    pk2, t2 = sb.giant(sb.GEN_BWD_MAX_ATOMS + 1)
    rb = eng.upload(pk2)  # (within the upload limit)
    with pytest.raises(_hip.ScannHipError) as ei:
        eng.train_forward(rb, t2)
    assert ei.value.code == -2 and "LDS" in str(ei.value), str(ei.value)
    with pytest.raises(_hip.ScannHipError):
        eng.train_backward(rb, 1.0, pk2.n_struct)  # nothing was kept for it
    rb.free()
    g1, w1 = eng.get_grads(), eng.get_weights()
    assert all(np.array_equal(g0[k], g1[k]) and np.array_equal(w0[k], w1[k]) for k in g0)
    s1 = eng.train_forward(rb_small, t_small)
    eng.zero_grads()
    eng.train_backward(rb_small, s1, small.n_struct)
    g2 = eng.get_grads()
    assert s1 == s0 and all(np.array_equal(g0[k], g2[k]) for k in g0)  # (no atomics on this path: the same bits)
    rb_small.free()

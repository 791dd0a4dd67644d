"""GPU tests of fine-tuning (scann_set_lr_scale): frozen tensors keep their bytes, trained tensors get the bytes of the whole backward and
of the unscaled optimiser, the backward really stops at the floor (zero gradient entries below it, scann_train_stages), on the fused and
the modular chain, in the one-call step with two steps in flight, on the plain-fp32 kernels, and end to end through train.py.
Deterministic mode unless a test says otherwise: bit equality is then the claim, not a tolerance."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import scann_oracle as so

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location("_ft_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tg = _load("test_gpu_training")  # check_grads, grad_reference, setup_widths, OTHER_WIDTHS, _write_dataset
host = _load("test_finetune_host")  # stage_of: the stage table, restated

VARIANTS = {
    "scann_plus": dict(),
    "base": dict(g_update=False),
    "ring_cgcnn": dict(use_ring=True, feature="cgcnn"),
    "e_b": dict(),
}
_CASES = {}


def case(variant, L, n=12):
    """(cfg, weights, packed batch of n <= 16 structures, targets) of one architecture variant; built once"""
    key = (variant, L, n)
    if key not in _CASES:
        from scann import _hip

        cfg = so.default_config("qm9")
        cfg["model"]["n_attention"] = L
        cfg["model"].update(VARIANTS[variant])
        if variant == "e_b":
            cfg["hyper"]["target"] = "e_b"
        ring, cg = bool(cfg["model"].get("use_ring")), cfg["model"].get("feature") == "cgcnn"
        w = so.init_weights(cfg, 8, perturb=True)
        de, dn = so.synth_dataset(n, 3, use_ring=ring)
        inputs, targets = so.pad_batch(de, dn, cfg["model"]["g_update"], use_ring=ring)
        if cg:
            table = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")
            inputs["atomic"] = table[inputs["atomic"]]
        _CASES[key] = (cfg, w, _hip.pack_inputs(inputs), np.asarray(targets, np.float32))
    return _CASES[key]


def floor_scale(w, L, f):
    """the scale of floor f: 1 for every tensor of a stage >= f, 0 below"""
    return {n: 1.0 if host.stage_of(n, L) >= f else 0.0 for n in w}


def engine(cfg, w, deterministic=True):
    from scann.models.scann_model import HipModel

    eng = HipModel(cfg, w, device=0, deterministic=deterministic).engine
    eng.train_begin()
    return eng


def one_backward(cfg, w, pk, targets, scale, lr=5e-4):
    """train_forward / zero_grads / train_backward / adam_step under `scale` on a fresh handle
    -> (raw gradients, stages that ran, weights after the step)"""
    eng = engine(cfg, w)
    eng.set_lr_scale(scale)
    rb = eng.upload(pk)
    sse = eng.train_forward(rb, targets, dropout=0.1, seed=5)
    eng.zero_grads()
    eng.train_backward(rb, sse, pk.n_struct)
    raw, stages = eng.get_grads(masked=False), eng.train_stages()
    masked = eng.get_grads()
    for k in raw:  # get_grads(masked=True), the default: zeros for every frozen tensor, the raw entries otherwise
        assert np.array_equal(masked[k], raw[k] if scale is None or scale[k] > 0 else np.zeros_like(raw[k])), k
    eng.adam_step(lr)
    wts = eng.get_weights()
    rb.free()
    eng.close()
    return raw, stages, wts


def check_floor(cfg, w, L, f, full, cut):
    """cases 2 and 3 of one floor: `full` the all-trainable run, `cut` the run under floor_scale(f)"""
    g_full, st_full, w_full = full
    g_cut, st_cut, w_cut = cut
    assert st_full == list(range(L + 3))
    assert st_cut == list(range(f, L + 3)), (f, st_cut)  # no bit below the floor, every bit at and above it
    below_nonzero = 0
    for k in w:
        st = host.stage_of(k, L)
        if st >= f:  # trained: the whole backward's bytes, and the whole step's
            assert np.array_equal(g_cut[k], g_full[k]), (f, k)
            assert np.array_equal(w_cut[k], w_full[k]), (f, k)
        else:  # below the floor: never written; frozen: never applied
            assert not g_cut[k].any(), (f, k)
            assert np.array_equal(w_cut[k], w[k]), (f, k)
            below_nonzero += bool(g_full[k].any())
    if f > 0:
        assert below_nonzero > 0  # ... where the all-trainable run has gradients


# ---- 2 + 3. trained tensors get the full step's bytes; the floor is real -------------------------------------------------------

@pytest.mark.parametrize("L,floors", [(2, (0, 1, 2, 3, 4)), (7, (0, 4, 9))], ids=["L2", "L7"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_backward_stops_at_the_floor_and_keeps_the_trained_bytes(hip_lib, variant, L, floors):
    cfg, w, pk, targets = case(variant, L)
    full = one_backward(cfg, w, pk, targets, None)
    assert any(not np.array_equal(full[2][k], w[k]) for k in w)
    for f in floors:
        check_floor(cfg, w, L, f, full, one_backward(cfg, w, pk, targets, floor_scale(w, L, f)))


# ---- 4. both chains ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["scann_plus", "base"])
def test_modular_backward_stops_at_the_floor(hip_lib, monkeypatch, variant):
    monkeypatch.setenv("SCANN_TRAIN_FUSED", "0")
    L = 2
    cfg, w, pk, targets = case(variant, L)
    full = one_backward(cfg, w, pk, targets, None)
    for f in (L, L + 2):
        check_floor(cfg, w, L, f, full, one_backward(cfg, w, pk, targets, floor_scale(w, L, f)))


# ---- 1. frozen means untouched ------------------------------------------------------------------------------------------------

def _three_steps(eng, rb, targets):
    return [eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=i) for i in range(3)]


def _frozen_means_untouched(cfg, w, pk, targets, L):
    body = floor_scale(w, L, L + 2)
    frozen = [k for k in w if body[k] == 0.0]
    assert frozen and len(frozen) < len(w)
    a = engine(cfg, w)
    a.set_lr_scale(body)
    assert a.lr_scale() == body
    rb = a.upload(pk)
    _three_steps(a, rb, targets)
    stages = a.train_stages()
    wa = a.get_weights()
    for k in w:
        assert np.array_equal(wa[k], w[k]) == (k in frozen), k
    # the moments of the frozen tensors are untouched too: with the scale cleared, optimiser steps on zero gradients without the
    # regulariser move a weight by m / (sqrt(v) + eps) alone
    a.set_lr_scale(None)
    for _ in range(2):
        a.zero_grads()
        a.adam_step(1e-3, l2=0.0)
    wp = a.get_weights()
    for k in w:
        assert np.array_equal(wp[k], w[k]) == (k in frozen), k
    rb.free()
    # a second handle, the scale set and cleared again: the same steps change those tensors
    b = engine(cfg, w)
    b.set_lr_scale(body)
    b.set_lr_scale(None)
    assert set(b.lr_scale().values()) == {1.0}
    rb = b.upload(pk)
    _three_steps(b, rb, targets)
    wb = b.get_weights()
    assert all(not np.array_equal(wb[k], w[k]) for k in frozen)
    rb.free()
    return stages, b.train_stages()


def test_frozen_means_untouched(hip_lib):
    L = 2
    cfg, w, pk, targets = case("scann_plus", L)
    stages, stages_clear = _frozen_means_untouched(cfg, w, pk, targets, L)
    assert stages == [L + 2] and stages_clear == list(range(L + 3))


# ---- 9. plain-fp32 handle -------------------------------------------------------------------------------------------------------

def test_frozen_means_untouched_on_the_plain_fp32_kernels(hip_lib):
    """64 / 4: the optimiser rule holds; that backward is not cut at the floor, and scann_train_stages says so"""
    cfg, w, pk, targets, _ = tg.setup_widths(tg.OTHER_WIDTHS["64x4"], n=12, seed=31)
    L = cfg["model"]["n_attention"]
    stages, stages_clear = _frozen_means_untouched(cfg, w, pk, np.asarray(targets, np.float32), L)
    assert stages == list(range(L + 3)) and stages_clear == list(range(L + 3))


# ---- 5. scale arithmetic ------------------------------------------------------------------------------------------------------

def test_scale_arithmetic(hip_lib):
    import torch_ref

    L = 2
    cfg, w, pk, targets = case("scann_plus", L)
    out = []
    for scale in (None, {k: 1.0 for k in w}):
        eng = engine(cfg, w)
        eng.set_lr_scale(scale)
        rb = eng.upload(pk)
        sse = _three_steps(eng, rb, targets)
        out.append((sse, eng.get_weights()))
        rb.free()
    assert out[0][0] == out[1][0]
    for k in w:  # a scale of all ones: the bytes of no scale
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    # s = 0.25 on one layer: its one-step update is the Keras update run with lr_hat * 0.25; the other tensors are the unscaled step's
    layer = [k for k in w if host.stage_of(k, L) == 2]
    scale = {k: 0.25 if k in layer else 1.0 for k in w}
    lr, b1, b2, eps = 5e-4, 0.9, 0.999, 1e-7
    g, _, w_plain = one_backward(cfg, w, pk, targets, None, lr=lr)
    g_s, stages, w_scaled = one_backward(cfg, w, pk, targets, scale, lr=lr)
    assert stages == list(range(L + 3))
    moved = 0
    for k in w:
        assert np.array_equal(g_s[k], g[k]), k
        if k not in layer:
            assert np.array_equal(w_scaled[k], w_plain[k]), k
            continue
        w64 = w[k].astype(np.float64)
        gi = g[k].astype(np.float64) + (2e-4 * w64 if k.endswith(torch_ref.REGULARIZED) else 0.0)
        m, v = (1 - b1) * gi, (1 - b2) * gi * gi
        lr_hat = lr * np.sqrt(1 - b2) / (1 - b1)
        want = w64 - lr_hat * 0.25 * m / (np.sqrt(v) + eps)
        assert np.allclose(w_scaled[k], want, rtol=1e-4, atol=2e-6), k  # the bound of test_adam_step_matches_keras_formula
        moved += int(np.sum(np.abs(w_scaled[k] - w_plain[k]) > 1e-5))
    assert moved > 1000  # (the unscaled step lies far outside that bound: the factor is really applied)


# ---- 6. non-deterministic mode -------------------------------------------------------------------------------------------------

def test_default_mode_gradients_above_the_floor_match_autograd(hip_lib):
    L = 2
    cfg, w, pk, targets = case("scann_plus", L)
    scale = floor_scale(w, L, L + 1)
    eng = engine(cfg, w, deterministic=False)
    eng.set_lr_scale(scale)
    rb = eng.upload(pk)
    sse = eng.train_forward(rb, targets, dropout=0.0, seed=1)
    eng.zero_grads()
    eng.train_backward(rb, sse, pk.n_struct)
    got = eng.get_grads()
    assert eng.train_stages() == [L + 1, L + 2]
    rb.free()
    rmse, ref, g32 = tg.grad_reference(cfg, w, pk, targets)
    live = [k for k in w if scale[k] > 0]
    assert len(live) == 10
    tg.check_grads(got, cfg, w, pk, targets, refs=(rmse, {k: ref[k] for k in live}, {k: g32[k] for k in live}))
    assert all(not got[k].any() for k in w if k not in live)


# ---- 7. fused step, two steps in flight, the floor changed between steps ------------------------------------------------------------

def test_steps_in_flight_and_floor_changes(hip_lib):
    from scann import _hip

    L = 2
    cfg, w, pk, targets = case("scann_plus", L)
    de, dn = so.synth_dataset(9, 77)
    inputs2, targets2 = so.pad_batch(de, dn, True)
    pk2, targets2 = _hip.pack_inputs(inputs2), np.asarray(targets2, np.float32)
    head, top, ones = floor_scale(w, L, L + 2), floor_scale(w, L, L), {k: 1.0 for k in w}
    # a: two steps in flight under the head-only floor, then the floor lowered (all ones), raised (top layer up), cleared
    a = engine(cfg, w)
    a.set_lr_scale(head)
    ra, ra2 = a.upload(pk), a.upload(pk2)
    a.train_step_begin(ra, targets, 1e-3, dropout=0.1, seed=0)
    a.train_step_begin(ra2, targets2, 1e-3, dropout=0.1, seed=1)
    with pytest.raises(RuntimeError, match="in flight"):
        a.set_lr_scale(ones)
    stats = [a.train_step_end()]
    with pytest.raises(RuntimeError, match="in flight"):
        a.set_lr_scale(None)
    stats.append(a.train_step_end())
    assert a.lr_scale() == head and a.train_stages() == [L + 2]
    w_a2 = a.get_weights()
    a.set_lr_scale(ones)
    stats.append(a.train_step(ra, targets, 1e-3, dropout=0.1, seed=2))
    assert a.train_stages() == list(range(L + 3))
    a.set_lr_scale(top)
    stats.append(a.train_step(ra2, targets2, 1e-3, dropout=0.1, seed=3))
    assert a.train_stages() == [L, L + 1, L + 2]
    a.set_lr_scale(None)
    stats.append(a.train_step(ra, targets, 1e-3, dropout=0.1, seed=4))
    w_a = a.get_weights()
    # b: the same five steps as separate calls, one at a time
    b = engine(cfg, w)
    rb_, rb2 = b.upload(pk), b.upload(pk2)
    w_b2 = None
    for i, (scale, (r, t)) in enumerate(zip((head, head, ones, top, None), ((rb_, targets), (rb2, targets2)) * 3)):
        b.set_lr_scale(scale)
        sse = b.train_forward(r, t, dropout=0.1, seed=i)
        b.zero_grads()
        b.train_backward(r, sse, len(t))
        b.adam_step(1e-3)
        assert sse == stats[i][0] and len(t) == stats[i][1], (i, sse, stats[i])
        if i == 1:
            w_b2 = b.get_weights()
    w_b = b.get_weights()
    for k in w:
        assert np.array_equal(w_a2[k], w_b2[k]), k  # the two steps in flight = the six separate calls
        assert np.array_equal(w_a[k], w_b[k]), k
        assert np.array_equal(w_a2[k], w[k]) == (head[k] == 0.0), k
    for r in (ra, ra2, rb_, rb2):
        r.free()
    # refused arguments leave the scale as it was
    for bad in (dict(ones, **{"after_Lc/bias": -0.5}), dict(ones, **{"after_Lc/bias": float("nan")}),
                dict(ones, **{"after_Lc/bias": float("inf")}), {k: 0.0 for k in w}):
        with pytest.raises(RuntimeError, match="scale"):
            b.set_lr_scale(bad)
    with pytest.raises(ValueError, match="no_such_tensor"):
        b.set_lr_scale({"no_such_tensor/kernel": 1.0})
    assert set(b.lr_scale().values()) == {1.0}


def test_scale_survives_train_begin(hip_lib):
    """set before scann_train_begin: it takes effect in the first step"""
    from scann.models.scann_model import HipModel

    L = 2
    cfg, w, pk, targets = case("scann_plus", L)
    head = floor_scale(w, L, L + 2)
    eng = HipModel(cfg, w, device=0, deterministic=True).engine
    eng.set_lr_scale(head)
    eng.train_begin()
    assert eng.lr_scale() == head
    rb = eng.upload(pk)
    eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=0)
    got = eng.get_weights()
    assert eng.train_stages() == [L + 2]
    for k in w:
        assert np.array_equal(got[k], w[k]) == (head[k] == 0.0), k
    rb.free()


# ---- 8. non-interference ------------------------------------------------------------------------------------------------------

def test_scale_does_not_reach_anything_but_training(hip_lib):
    from scann.models.scann_model import HipModel

    L = 2
    cfg, w, pk, targets = case("scann_plus", L)
    model = HipModel(cfg, w, device=0, deterministic=True)
    eng = model.engine
    eng.train_begin()
    index = model.build_index(pk)

    def snapshot():
        rb = eng.upload(pk)
        ig = eng.input_grads(rb)
        sse = eng.train_forward(rb, targets, dropout=0.0, seed=0)
        rb.free()
        near = model.nearest(pk, index, k=3)
        return ig, sse, model.predict(pk), near

    before = snapshot()
    eng.set_lr_scale(floor_scale(w, L, L + 2))
    stages = eng.train_stages()
    after = snapshot()
    assert eng.train_stages() == stages  # scann_input_grads runs the whole backward and does not count as a training backward
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), k
    assert before[0]["neighbor_distance"].any()  # (it reached the leaves)
    assert before[1] == after[1]
    assert np.array_equal(before[2], after[2])
    for k in before[3]:
        assert np.array_equal(before[3][k], after[3][k]), k


# ---- 10. end to end ---------------------------------------------------------------------------------------------------------

def test_cli_fine_tune_from_a_checkpoint(hip_lib, tmp_path):
    """train.py for two epochs, then train.py --pretrained with the body frozen and the head drawn afresh; predict_model.py loads it"""
    import yaml

    from scann.models.scann_model import _read_container

    e_path, n_path = tg._write_dataset(tmp_path, n=64)
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 1
    cfg["hyper"].update(batch_size=16, test_percent=0.125, scaler=True, scheduler="sgdr", train_size="", test_size="",
                        data_size=64, data_nei_path=n_path, data_energy_path=e_path, lr=2e-3, min_lr=2e-4, pretrained="")
    cfg["model"].pop("feature"); cfg["model"].pop("use_drop"); cfg["hyper"].pop("target")  # the CLI injects these
    runs = {}
    for name, extra in (("pre", []), ("fine", ["--pretrained", str(tmp_path / "pre_homo" / "models" / "model_homo.h5"),
                                               "--freeze", "embed_atom/*,dense_embed/*,neighbor_?/*,local_attention_*,residual_norm_*,"
                                               "after_Lc/*,global_attention/*", "--reset", "bf_property/*,predict_property/*"])):
        c = {"model": dict(cfg["model"]), "hyper": dict(cfg["hyper"], save_path=str(tmp_path / name))}
        ypath = tmp_path / (name + ".yaml")
        yaml.safe_dump(c, open(ypath, "w"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "homo", str(ypath), "--epochs", "2", "--seed", "7",
                            "--deterministic", "True"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (r.stdout, _read_container(str(tmp_path / (name + "_homo") / "models" / "model_homo.h5"))[1])
    pre, fine = runs["pre"][1], runs["fine"][1]
    head = [k for k in pre if k.startswith(("bf_property/", "predict_property/"))]
    assert len(head) == 4 and sorted(pre) == sorted(fine)
    for k in pre:
        assert np.array_equal(pre[k], fine[k]) == (k not in head), k
    n_total = sum(v.size for v in pre.values())
    n_head = sum(pre[k].size for k in head)
    assert "Trainable params: {:,} / {:,}".format(n_total, n_total) in runs["pre"][0]
    assert "Trainable params: {:,} / {:,}".format(n_head, n_total) in runs["fine"][0]
    assert "re-initialised 4 tensors" in runs["fine"][0]
    saved = yaml.safe_load(open(tmp_path / "fine_homo" / "config.yaml"))
    assert saved["hyper"]["reset"] == ["bf_property/*", "predict_property/*"] and len(saved["hyper"]["freeze"]) == 7
    assert saved["hyper"]["lr_scale"] is None
    out = str(tmp_path / "fine_homo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict_model.py"), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(out + "/energy_pre_homo.pickle")

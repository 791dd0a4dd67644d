"""GPU: the deterministic training mode (scann_set_deterministic, Engine.set_deterministic, hyper.deterministic, train.py
--deterministic).  With it on, the six small reductions that otherwise end in float atomics (readout bias, basis MLP, base-branch
filter_geo, species table, dense_embed, ring / cgcnn embedding) add per-workgroup slots in a fixed order, so:
  1. repeated backward passes over one batch give bitwise-equal gradients, on every branch and on both backward schedules;
  2. only the tensors of those reductions differ from the default mode, and only by rounding;
  3. the gradients still pass the suite's fp64-autograd rule;
  4. training steps, serial or two in flight, give bitwise-equal weights, Adam state and SSE;
  5. two whole train.py runs give bitwise-equal checkpoints and identical epoch lines;
  6. nothing else changes: plain-fp32 handles, inference, switching between steps, device memory."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scann_oracle as so
import size_batches as sb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location("_det_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tg = _load("test_gpu_training")  # check_grads, setup_widths, OTHER_WIDTHS, _write_dataset

# the gradient tensors the six reductions write (test_gpu_training.py's list of float-atomic tensors)
FLOAT_ATOMIC = ("embed_atom/", "dense_embed/", "neighbor_d/", "neighbor_w/", "predict_property/", "extra_embed/")
# g_update=False: each layer's filter_geo goes through base_geom_bwd_kernel
BASE_FILTER = re.compile(r"local_attention_\d+/filter_geo/")


def _atomic_tensor(name, g_update):
    return name.startswith(FLOAT_ATOMIC) or (not g_update and BASE_FILTER.match(name) is not None)


def _qm9_b128_L7():
    from scann import _hip

    de, dn = so.synth_dataset(128, 11)
    inputs, targets = so.pad_batch(de, dn, True)
    return _hip.pack_inputs(inputs), np.asarray(targets, np.float32)


def _case(name):
    """(cfg, weights, packed batch, targets) of one branch of the repeat tests"""
    from scann import _hip

    cfg = so.default_config("mp2018" if name == "mp2018_b128" else "qm9")
    if name == "qm9_b128_L7":
        cfg["model"]["n_attention"] = 7
        pk, t = _qm9_b128_L7()
    elif name == "mp2018_b128":
        cfg["model"]["n_attention"] = 2
        pk, t = sb.mp2018_b128()
    elif name == "qm9_b260":
        cfg["model"]["n_attention"] = 2
        pk, t = sb.qm9_b260()
    elif name == "base":
        cfg["model"].update(n_attention=3, g_update=False)
        de, dn = so.synth_dataset(96, 13)
        inputs, t = so.pad_batch(de, dn, False)
        pk = _hip.pack_inputs(inputs)
    elif name == "ring_cgcnn":
        cfg["model"].update(n_attention=2, use_ring=True, feature="cgcnn")
        de, dn = so.synth_dataset(64, 3, use_ring=True)
        inputs, t = so.pad_batch(de, dn, True, use_ring=True)
        table = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")
        inputs["atomic"] = table[inputs["atomic"]]
        pk = _hip.pack_inputs(inputs)
    elif name == "e_b":
        cfg["model"]["n_attention"] = 2
        cfg["hyper"]["target"] = "e_b"
        de, dn = so.synth_dataset(64, 21)
        inputs, t = so.pad_batch(de, dn, True)
        pk = _hip.pack_inputs(inputs)
    else:
        raise KeyError(name)
    w = so.init_weights(cfg, 3, perturb=True)
    return cfg, w, pk, np.asarray(t, np.float32)


CASES = ["qm9_b128_L7", "mp2018_b128", "qm9_b260", "base", "ring_cgcnn", "e_b"]


def _grads(eng, rb, pk, targets, n, dropout=0.1, seed=5):
    out = []
    for _ in range(n):
        sse = eng.train_forward(rb, targets, dropout=dropout, seed=seed)
        eng.zero_grads()
        eng.train_backward(rb, sse, pk.n_struct)
        out.append(eng.get_grads())
    return out


def _equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


# ---- 1 + 2. repeated backward: bitwise equal in the mode; only the six reductions differ from the default --------------------

@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "modular"])
@pytest.mark.parametrize("name", CASES)
def test_repeated_backward_is_bitwise_equal(hip_lib, monkeypatch, name, fused):
    from scann.models.scann_model import HipModel

    monkeypatch.setenv("SCANN_TRAIN_FUSED", fused)
    cfg, w, pk, targets = _case(name)
    model = HipModel(cfg, w, device=0)
    eng = model.engine
    eng.train_begin()
    rb = eng.upload(pk)
    default = _grads(eng, rb, pk, targets, 5)
    eng.set_deterministic(True)
    det = _grads(eng, rb, pk, targets, 20)
    rb.free()
    ref = det[0]
    for i, g in enumerate(det[1:], 1):
        bad = [k for k in ref if not np.array_equal(ref[k], g[k])]
        assert not bad, (name, i, bad)
    g_update = bool(cfg["model"]["g_update"])
    differed = sum(not _equal(default[0], g) for g in default[1:])
    print("%s fused=%s: %d of %d default-mode repeats differed from the first (float atomics); deterministic: 20 equal"
          % (name, fused, differed, len(default) - 1))
    # 2. outside the six reductions the bits are the default mode's; inside, rounding only (the existing tests' bound)
    for k in ref:
        if _atomic_tensor(k, g_update):
            assert np.allclose(ref[k], default[0][k], rtol=1e-4, atol=1e-7), k
        else:
            assert np.array_equal(ref[k], default[0][k]), k


# ---- 3. accuracy: the fp64-autograd rule of the suite ---------------------------------------------------------------------

@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "modular"])
@pytest.mark.parametrize("over", [dict(n_attention=7), dict(g_update=False), dict(use_ring=True, feature="cgcnn"), dict(target="e_b")],
                         ids=["qm9_L7", "base", "ring_cgcnn", "e_b"])
def test_deterministic_gradients_match_autograd(hip_lib, monkeypatch, over, fused):
    from scann import _hip
    from scann.models.scann_model import HipModel

    monkeypatch.setenv("SCANN_TRAIN_FUSED", fused)
    over = dict(over)
    target = over.pop("target", None)
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 2
    cfg["model"].update(over)
    if target:
        cfg["hyper"]["target"] = target
    ring, cg = bool(cfg["model"].get("use_ring")), cfg["model"].get("feature") == "cgcnn"
    w = so.init_weights(cfg, 8, perturb=True)
    de, dn = so.synth_dataset(12, 3, use_ring=ring)
    inputs, targets = so.pad_batch(de, dn, cfg["model"]["g_update"], use_ring=ring)
    if cg:
        table = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")
        inputs["atomic"] = table[inputs["atomic"]]
    pk = _hip.pack_inputs(inputs)
    model = HipModel(cfg, w, device=0, deterministic=True)
    eng = model.engine
    eng.train_begin()
    rb = eng.upload(pk)
    (got,) = _grads(eng, rb, pk, targets, 1, dropout=0.0)
    rb.free()
    tg.check_grads(got, cfg, w, pk, targets)


def test_deterministic_size_batch_gradients_match_autograd(hip_lib):
    """qm9_b260 (the large side of the attention-backward switch) in the mode, against fp64 autograd"""
    from scann.models.scann_model import HipModel

    cfg, w, pk, targets = _case("qm9_b260")
    eng = HipModel(cfg, w, device=0, deterministic=True).engine
    eng.train_begin()
    rb = eng.upload(pk)
    (got,) = _grads(eng, rb, pk, targets, 1, dropout=0.0)
    rb.free()
    tg.check_grads(got, cfg, w, pk, targets)


# ---- 4. training steps ---------------------------------------------------------------------------------------------------

def _adam_probe(eng):
    """two optimiser steps on zero gradients: the weights then move by m / (sqrt(v) + eps) alone, so equal bits after them say the
    two handles' Adam moments are equal as well"""
    for _ in range(2):
        eng.zero_grads()
        eng.adam_step(1e-3)
    return eng.get_weights()


def test_training_steps_are_bitwise_equal(hip_lib):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg, w, pk, targets = _case("qm9_b128_L7")
    cfg["model"]["n_attention"] = 3
    de, dn = so.synth_dataset(40, 77)
    inputs2, targets2 = so.pad_batch(de, dn, True)
    pk2 = _hip.pack_inputs(inputs2)
    batches = [(pk, targets), (pk2, np.asarray(targets2, np.float32))]
    runs = []
    for _ in range(2):
        eng = HipModel(cfg, w, device=0, deterministic=True).engine
        eng.train_begin()
        rbs = [eng.upload(b) for b, _ in batches]
        sse = [eng.train_step(rbs[i % 2], batches[i % 2][1], 1e-3, dropout=0.1, seed=i) for i in range(10)]
        wts = eng.get_weights()
        probe = _adam_probe(eng)
        runs.append((sse, wts, probe))
        for rb in rbs:
            rb.free()
    assert runs[0][0] == runs[1][0]
    assert _equal(runs[0][1], runs[1][1]) and _equal(runs[0][2], runs[1][2])

    # two steps in flight = one at a time, bit for bit
    results = {}
    for mode in ("serial", "pipelined"):
        eng = HipModel(cfg, w, device=0, deterministic=True).engine
        eng.train_begin()
        stats, pending = [], []
        for i in range(6):
            b, t = batches[i % 2]
            rb = eng.upload(b)
            eng.train_step_begin(rb, t, 1e-3, dropout=0.1, seed=i)
            pending.append(rb)
            if mode == "serial" or len(pending) == 2:
                stats.append(eng.train_step_end())
                pending.pop(0).release()
        while pending:
            stats.append(eng.train_step_end())
            pending.pop(0).release()
        results[mode] = (stats, eng.get_weights(), _adam_probe(eng))
    assert results["serial"][0] == results["pipelined"][0]
    assert _equal(results["serial"][1], results["pipelined"][1]) and _equal(results["serial"][2], results["pipelined"][2])


# ---- 5. whole training runs ----------------------------------------------------------------------------------------------

def test_cli_training_runs_are_bitwise_equal(hip_lib, tmp_path):
    import yaml

    from scann.models.scann_model import _read_container

    e_path, n_path = tg._write_dataset(tmp_path, n=64)
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 2
    cfg["model"]["use_drop"] = True
    outs = []
    for run in range(2):
        c = {"model": dict(cfg["model"]), "hyper": dict(cfg["hyper"])}
        c["hyper"].update(batch_size=16, test_percent=0.125, scaler=True, scheduler="sgdr", train_size="", test_size="",
                          data_size=64, data_nei_path=n_path, data_energy_path=e_path, lr=2e-3, min_lr=2e-4,
                          save_path=str(tmp_path / ("run%d" % run)), pretrained="")
        c["model"].pop("feature"); c["model"].pop("use_drop"); c["hyper"].pop("target")  # the CLI injects these
        ypath = tmp_path / ("cfg%d.yaml" % run)
        yaml.safe_dump(c, open(ypath, "w"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "homo", str(ypath), "--epochs", "3", "--seed", "7",
                            "--use_drop", "True", "--deterministic", "True"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        epochs = [re.sub(r" - \d+s - ", " - ", ln) for ln in r.stdout.splitlines() if ln.startswith("Epoch ")]
        assert len(epochs) == 3, r.stdout[-2000:]
        _, weights = _read_container(str(tmp_path / ("run%d_homo" % run) / "models" / "model_homo.h5"))
        outs.append((epochs, weights))
    assert outs[0][0] == outs[1][0]
    assert sorted(outs[0][1]) == sorted(outs[1][1])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


# ---- 6. no side effects ----------------------------------------------------------------------------------------------------

def test_plain_fp32_handle_trains_to_the_same_bits(hip_lib):
    """64 / 4: the plain-fp32 kernels are fixed-order already; the flag is accepted and changes nothing"""
    from scann.models.scann_model import HipModel

    cfg, w, pk, targets, _ = tg.setup_widths(tg.OTHER_WIDTHS["64x4"], n=20, seed=31)
    out = []
    for on in (False, True):
        eng = HipModel(cfg, w, device=0, deterministic=on).engine
        eng.train_begin()
        rb = eng.upload(pk)
        sse = [eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=i) for i in range(3)]
        out.append((sse, eng.get_weights()))
        rb.free()
    assert out[0][0] == out[1][0] and _equal(out[0][1], out[1][1])


def test_inference_bytes_do_not_depend_on_the_flag(hip_lib):
    from scann.models.scann_model import HipModel

    cfg, w, pk, _ = _case("qm9_b128_L7")
    model = HipModel(cfg, w, device=0, infer=True)
    y0, ga0 = model.predict(pk)
    model.engine.set_deterministic(True)
    y1, ga1 = model.predict(pk)
    assert y0.tobytes() == y1.tobytes() and ga0.tobytes() == ga1.tobytes()


def test_switching_the_flag_between_steps(hip_lib):
    """off -> on -> off between steps: each step does what its mode does -- the deterministic one equals a step of a handle that
    was deterministic from the start, bit for bit, and the handle keeps training afterwards"""
    from scann.models.scann_model import HipModel

    cfg, w, pk, targets = _case("e_b")
    a = HipModel(cfg, w, device=0).engine
    a.train_begin()
    rba = a.upload(pk)
    g_off = _grads(a, rba, pk, targets, 1)[0]
    a.set_deterministic(True)
    g_on = _grads(a, rba, pk, targets, 2)
    a.set_deterministic(False)
    g_off2 = _grads(a, rba, pk, targets, 1)[0]
    b = HipModel(cfg, w, device=0, deterministic=True).engine
    b.train_begin()
    rbb = b.upload(pk)
    g_ref = _grads(b, rbb, pk, targets, 1)[0]
    assert _equal(g_on[0], g_ref) and _equal(g_on[1], g_ref)
    for g in (g_off, g_off2):
        for k in g_ref:
            assert np.allclose(g[k], g_ref[k], rtol=1e-4, atol=1e-7), k
    sse = a.train_step(rba, targets, 1e-3, dropout=0.1, seed=9)
    assert np.isfinite(sse[0])
    rba.free()
    rbb.free()


def test_deterministic_steps_do_not_eat_device_memory(hip_lib):
    """fresh batches every step: the slots are allocated with each batch's workspace and freed with it"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 2
    w = so.init_weights(cfg, 3, perturb=True)
    eng = HipModel(cfg, w, device=0, deterministic=True).engine
    eng.train_begin()
    batches = []
    for n, seed in ((6, 1), (40, 2), (17, 3), (64, 4)):
        de, dn = so.synth_dataset(n, seed)
        inputs, t = so.pad_batch(de, dn, True)
        batches.append((_hip.pack_inputs(inputs), np.asarray(t, np.float32)))

    def round_():
        for i, (pk, t) in enumerate(batches):
            rb = eng.upload(pk)
            eng.train_step(rb, t, 1e-4, dropout=0.1, seed=i)
            rb.free()

    round_()
    free0, _ = eng.device_memory()
    for _ in range(10):
        round_()
    free1, _ = eng.device_memory()
    assert free0 - free1 <= 32 << 20, (free0, free1)

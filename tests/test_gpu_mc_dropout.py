"""GPU tests of Monte Carlo dropout (scann_predict_mc / HipModel.predict_uncertainty): every sample against the torch fp64 graph run
with the same structure-local masks (tests/mc_ref.py) under test_gpu_parity's bound for y, the device reduction against NumPy's, and
the call's promises -- batch invariance, bit-reproducibility, no effect on the handle -- plus the refusals."""
import ctypes as C

import numpy as np
import pytest

import mc_ref
import scann_oracle as so
from test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu


def setup(n=6, seed=1, L=2, target=None, widths=None, **over):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if widths:
        cfg["model"].update(widths)
        cfg["model"]["n_atoms"] = 100
    if target:
        cfg["hyper"]["target"] = target
    ring, cg = bool(cfg["model"]["use_ring"]), cfg["model"]["feature"] == "cgcnn"
    w = so.init_weights(cfg, 3, perturb=True)
    de, dn = so.synth_dataset(n, seed, use_ring=ring)
    inputs, _ = so.pad_batch(de, dn, cfg["model"]["g_update"], use_ring=ring)
    if cg:
        inputs["atomic"] = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")[inputs["atomic"]]
    return cfg, w, inputs, _hip.pack_inputs(inputs), HipModel(cfg, w, device=0, infer=True)


CASES = {
    "g_update": {},
    "g_update_L7": dict(L=7),
    "base": dict(g_update=False),
    "base_L7": dict(g_update=False, L=7),
    "no_attn_norm": dict(use_attn_norm=False),
    "no_ga_norm": dict(use_ga_norm=False),
    "use_drop": dict(use_drop=True),
    "base_use_drop": dict(g_update=False, use_drop=True),
    "ring": dict(use_ring=True),
    "cgcnn": dict(feature="cgcnn"),
    "e_b": dict(target="e_b"),
    "64x4": dict(widths=dict(local_dim=64, num_head=4, global_dim=96, dense_out=32), use_drop=True),
    # embedding rate 0: the MC fused-basis edge kernel reads the first layer from the per-species tables (tests/test_gpu_mc_sizes.py: 64 rows)
    "tables_attn_only": dict(use_drop=True, p_drop=0.0),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_sample_matches_the_oracle(hip_lib, monkeypatch, case):
    import torch_ref

    kw = dict(CASES[case])
    p_drop = kw.pop("p_drop", 0.1)
    cfg, w, _, pk, model = setup(**kw)
    T, seed = 3, 11
    keys = (np.arange(pk.n_struct) * 7 + 1).astype(np.uint64)
    p_attn = 0.05 if cfg["model"].get("use_drop") else 0.0
    rb = model.engine.upload(pk)
    r = model.engine.predict_mc(rb, T, seed=seed, keys=keys, p_drop=p_drop, p_attn=p_attn, want_samples=True)
    rb.free()
    ys = r["y_samples"]
    assert ys.shape == (T, pk.n_struct)
    ga64s = []
    for t in range(T):
        y64, ga64 = mc_ref.sample_ref(cfg, w, pk, seed, t, keys, p_drop, p_attn, monkeypatch)
        monkeypatch.setattr(torch_ref, "drop_scale_np", mc_ref.local_drop_twin(pk, t, keys, cfg["model"]["local_dim"]))
        y32 = np.asarray(torch_ref.forward_packed(cfg, w, pk, "float32", drop=(seed, p_drop) if p_drop > 0 else None,
                                                  attn_scale=mc_ref.attn_scales(pk, seed, t, keys, cfg["model"]["num_head"],
                                                                                cfg["model"]["n_attention"], p_attn))[0]).ravel()
        assert rel_err(ys[t], y64) <= max(RTOL, 2 * rel_err(y32, y64)), (t, rel_err(ys[t], y64), rel_err(y32, y64))
        ga64s.append(ga64)
    assert not np.array_equal(ys[0], ys[1])  # the samples differ
    # the device reduction: fp64 mean and unbiased std of the returned samples, to 1 ulp of fp32
    s64 = ys.astype(np.float64)
    for got, ref in ((r["y_mean"], s64.mean(0)), (r["y_std"], s64.std(0, ddof=1))):
        ref32 = ref.astype(np.float32)
        assert np.all(np.abs(got - ref32) <= np.spacing(np.abs(ref32))), (got, ref32)
    # GA mean / std against the oracle's per-sample scores
    g = np.stack(ga64s)
    assert rel_err(r["ga_mean"], g.mean(0)) <= 10 * RTOL
    assert np.max(np.abs(r["ga_std"] - g.std(0, ddof=1))) <= 10 * RTOL * max(float(np.abs(g).max()), 1e-30)


def test_batch_invariance(hip_lib):
    """permuting the structures (with or without their keys) permutes the results bitwise; a structure alone gives the bits it gets in
    a mixed batch; batch_size slicing changes nothing"""
    from scann import _hip

    cfg, w, inputs, pk, model = setup(n=9, seed=4, use_drop=True)
    B = pk.n_struct
    perm = np.random.default_rng(0).permutation(B)
    keys = np.arange(B) * 13 + 5
    kw = dict(samples=4, seed=21, return_samples=True)
    base = model.predict_uncertainty(inputs, keys=keys, **kw)
    pin = {k: np.asarray(v)[perm] for k, v in inputs.items()}
    got = model.predict_uncertainty(pin, keys=keys[perm], **kw)
    for k in ("predict_property", "predict_property_std", "global_attention", "global_attention_std"):
        assert np.array_equal(got[k], base[k][perm]), k
    assert np.array_equal(got["samples"], base["samples"][:, perm])
    nokey = model.predict_uncertainty(inputs, **kw)
    nokey_p = model.predict_uncertainty(pin, **kw)
    assert np.array_equal(nokey_p["samples"], nokey["samples"][:, perm])
    sliced = model.predict_uncertainty(inputs, keys=keys, batch_size=2, **kw)
    for k in base:
        assert np.array_equal(sliced[k], base[k]), k
    for s in (0, 4, B - 1):
        alone = model.predict_uncertainty(_hip.slice_packed(pk, s, s + 1), keys=keys[s:s + 1], **kw)
        assert np.array_equal(alone["samples"][:, 0], base["samples"][:, s])


def test_reproducible_seeded_and_rate_zero_is_the_plain_forward(hip_lib):
    cfg, w, inputs, pk, model = setup(n=8, seed=2)
    a = model.predict_uncertainty(inputs, samples=5, seed=3, return_samples=True)
    b = model.predict_uncertainty(inputs, samples=5, seed=3, return_samples=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    c = model.predict_uncertainty(inputs, samples=5, seed=4, return_samples=True)
    assert not np.array_equal(a["samples"], c["samples"])
    z = model.predict_uncertainty(inputs, samples=3, rate=0.0, attention_rate=0.0, return_samples=True)
    y, ga = model.predict(inputs)
    for t in range(3):
        assert np.array_equal(z["samples"][t], y)
    assert np.all(z["predict_property_std"] == 0) and np.array_equal(z["predict_property"], y)
    assert np.array_equal(z["global_attention"], ga) and np.all(z["global_attention_std"] == 0)


def test_handles_are_untouched(hip_lib):
    """an inference handle predicts the same bits afterwards; a training handle's gradients, weights and next (deterministic) step are
    those of a twin handle that never sampled"""
    from scann.models.scann_model import HipModel

    cfg, w, inputs, pk, model = setup(n=8, use_drop=True)
    y0, ga0 = model.predict(inputs)
    model.predict_uncertainty(inputs, samples=4)
    y1, ga1 = model.predict(inputs)
    assert np.array_equal(y0, y1) and np.array_equal(ga0, ga1)
    targets = np.linspace(-1, 1, pk.n_struct).astype(np.float32)
    a, b = HipModel(cfg, w, device=0, deterministic=True), HipModel(cfg, w, device=0, deterministic=True)
    res = []
    for i, m in enumerate((a, b)):
        eng = m.engine
        eng.train_begin()
        eng.set_attention_dropout(0.05)
        rb = eng.upload(pk)
        eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=3)
        sse = eng.train_forward(rb, targets, dropout=0.1, seed=4)
        eng.zero_grads()
        eng.train_backward(rb, sse, pk.n_struct)
        if i == 0:
            r = eng.predict_mc(rb, 4, seed=1)
            assert np.all(r["y_std"] > 0)
        grads, weights = eng.get_grads(), eng.get_weights()
        step = eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=5)
        res.append((grads, weights, step, eng.get_weights()))
        rb.free()
    (ga, wa, sa, wa2), (gb, wb, sb_, wb2) = res
    for k in ga:
        assert np.array_equal(ga[k].view(np.uint32), gb[k].view(np.uint32)), k
        assert np.array_equal(wa[k].view(np.uint32), wb[k].view(np.uint32)), k
        assert np.array_equal(wa2[k].view(np.uint32), wb2[k].view(np.uint32)), k
    assert sa == sb_


def test_refusals_at_the_abi(hip_lib):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg, w, inputs, pk, model = setup(n=4)
    w = dict(w)
    k = w["local_attention_0/query/kernel"].copy()
    k[3, 5] = 300.0
    w["local_attention_0/query/kernel"] = k
    ex = HipModel(cfg, w, device=0, infer=True)
    with pytest.raises(_hip.ScannHipError) as ei:
        ex.predict_uncertainty(pk, samples=2)
    assert ei.value.code == -2  # SCANN_ERR_UNSUPPORTED
    eng = model.engine
    rb = eng.upload(pk)
    B = pk.n_struct
    ym, ys = np.empty(B, np.float32), np.empty(B, np.float32)
    for T, pd, pa in ((1, 0.1, 0.0), (0, 0.1, 0.0), (4, 1.0, 0.0), (4, 1.5, 0.0), (4, 0.1, 1.0), (4, 0.1, 2.0)):
        r = eng.lib.scann_predict_mc(eng._h, rb._h, T, 0, None, pd, pa, ym.ctypes.data, ys.ctypes.data, None, None, None)
        assert r == -1, (T, pd, pa)  # SCANN_ERR_INVALID
    assert eng.lib.scann_predict_mc(eng._h, rb._h, 2, 0, None, -1.0, -1.0, ym.ctypes.data, ys.ctypes.data, None, None, None) == 0
    rb.free()


def test_default_rates_on_a_qm9_batch_and_the_scann_facade(hip_lib):
    from scann.models.scann_model import SCANN

    cfg, w, inputs, pk, model = setup(n=32, seed=7)
    r = model.predict_uncertainty(inputs, samples=32, seed=1)
    assert np.all(r["predict_property_std"] > 0) and np.all(np.isfinite(r["predict_property"]))
    s = SCANN.__new__(SCANN)
    s.model = model
    s.mean, s.std = 1.5, -2.0
    d = s.predict_uncertainty(inputs, samples=32, seed=1)
    assert np.array_equal(d["predict_property"], r["predict_property"] * np.float32(-2.0) + np.float32(1.5))
    assert np.array_equal(d["predict_property_std"], r["predict_property_std"] * np.float32(2.0))
    assert np.array_equal(d["global_attention"], r["global_attention"])

"""GPU: the outputs beyond y and the GlobalAttention scores -- every LocalAttention layer's attention weights (local_attention_<k>),
after_Lc and bf_property (scann_model.py:395-403, 423-442) -- against the NumPy oracle's intermediates (attn_local_<k+1>, after_Lc,
struc_rep), on every path that returns them, and y / GA scores unchanged by asking for them."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import scann_oracle as so

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # test_gpu_parity.py


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    scale = max(float(np.sqrt(np.mean(ref * ref))), 1e-30)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), scale)))


def all_names(cfg):
    return ["local_attention_%d" % k for k in range(cfg["model"]["n_attention"])] + ["after_Lc", "bf_property"]


def oracle_outputs(cfg, w, inputs, dtype=np.float32):
    inter = {}
    so.forward(cfg, w, inputs, dtype, intermediates=inter)
    amask = (np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0)
    ref = {"local_attention_%d" % k: inter["attn_local_%d" % (k + 1)] for k in range(cfg["model"]["n_attention"])}
    ref["after_Lc"] = inter["after_Lc"] * amask[..., None]  # padded atoms hold 0
    ref["bf_property"] = inter["struc_rep"]
    return ref


def check_against_oracle(cfg, w, inputs, got, names, fp64_bound=False, refs=None, measured=None):
    """every output against the fp32 oracle (whole padded arrays); fp64_bound: the bound of test_branches, max(RTOL, 2 x the fp32
    oracle's own error against fp64), for variants that are ill-conditioned in fp32.  refs: (oracle_outputs in fp32, in fp64 or None)
    of these very cfg / w / inputs, computed by the caller once for several calls; measured: a list that receives (name, rel_err,
    bound) of every output before it is asserted"""
    ref32 = refs[0] if refs else oracle_outputs(cfg, w, inputs)
    ref64 = (refs[1] if refs else oracle_outputs(cfg, w, inputs, np.float64)) if fp64_bound else None
    amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
    em = (np.asarray(inputs["neighbor_mask"]) != 0) & amask[:, :, None]
    has = em.any(-1)
    if fp64_bound:  # (in fp64 a logit + -1e9 keeps the logit: the 1/N rows are an fp32 convention, taken from the fp32 graph)
        for n in ref64:
            if n.startswith("local_attention_"):
                ref64[n].transpose(0, 2, 3, 1)[~has] = 1.0 / em.shape[2]
    for n, g in zip(names, got):
        assert g.shape == ref32[n].shape, (n, g.shape, ref32[n].shape)
        assert np.isfinite(g).all(), n
        if measured is not None:
            measured.append((n, rel_err(g, ref64[n]), max(RTOL, 2 * rel_err(ref32[n], ref64[n]))) if fp64_bound else (n, rel_err(g, ref32[n]), RTOL))
        if fp64_bound:
            assert rel_err(g, ref64[n]) <= max(RTOL, 2 * rel_err(ref32[n], ref64[n])), (n, rel_err(g, ref64[n]), rel_err(ref32[n], ref64[n]))
        else:
            assert rel_err(g, ref32[n]) <= RTOL, (n, rel_err(g, ref32[n]))
        if n.startswith("local_attention_"):
            a = g.transpose(0, 2, 3, 1)  # [B, M, N, H]
            assert not a[has[:, :, None] & ~em].any(), n  # masked slots of real atoms: exactly 0
            assert np.all(a[~has] == np.float32(1.0) / np.float32(em.shape[2])), n  # rows without a real neighbour: 1/N
            sums = a[has].astype(np.float64).sum(1)  # [rows, H]
            assert np.max(np.abs(sums - 1.0)) <= 1e-6, (n, np.max(np.abs(sums - 1.0)))
        if n == "after_Lc":
            assert not g[~amask].any()


def make(n=24, seed=0, kind="qm9", **over):
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    cfg["model"].update(over.pop("model", {}))
    cfg["hyper"].update(over.pop("hyper", {}))
    w = so.init_weights(cfg, 1234, perturb=True)
    de, dn = so.synth_dataset(n, seed, kind)
    inputs, _ = so.pad_batch(de, dn, g_update=cfg["model"]["g_update"])
    return cfg, w, inputs, HipModel(cfg, w, device=0, infer=True)


def test_every_output_matches_the_oracle_qm9(hip_lib):
    from scann import _hip

    cfg, w, inputs, model = make()
    inputs = {k: np.array(v) for k, v in inputs.items()}
    inputs["neighbor_mask"][3, 2, :] = False  # an isolated real atom: its rows hold 1/N, as the reference's
    names = all_names(cfg)
    got = model.predict(inputs, outputs=names)
    check_against_oracle(cfg, w, inputs, got, names)
    # a PackedBatch: the same numbers, packed
    pk = _hip.pack_inputs(inputs)
    packed = model.predict(pk, outputs=names)
    em = inputs["neighbor_mask"] & (inputs["atom_mask"][..., 0] != 0)[:, :, None]
    for n, g, p in zip(names, got, packed):
        if n.startswith("local_attention_"):
            assert p.shape == (pk.n_edge, 8) and np.array_equal(p, g.transpose(0, 2, 3, 1)[em])
        elif n == "after_Lc":
            assert p.shape == (pk.n_atom, 128) and np.array_equal(p, g[inputs["atom_mask"][..., 0] != 0])
        else:
            assert np.array_equal(p, g)


@pytest.mark.parametrize("over", [
    dict(model=dict(g_update=False)),
    dict(model=dict(use_attn_norm=False)),
    dict(model=dict(n_attention=1)),
    dict(hyper=dict(target="e_b")),
], ids=["base", "no_attn_norm", "L1", "e_b"])
def test_every_output_on_the_branches(hip_lib, over):
    cfg, w, inputs, model = make(n=12, seed=3, **{k: dict(v) for k, v in over.items()})
    names = all_names(cfg)
    check_against_oracle(cfg, w, inputs, model.predict(inputs, outputs=names), names, fp64_bound=True)


@pytest.mark.parametrize("g_update", [True, False], ids=["scann_plus", "base"])
def test_outputs_of_atoms_with_more_than_64_neighbours(hip_lib, g_update):
    """chunk tiles store exp(e - m_chunk); the merge scales them by the whole row's softmax state (built like
    test_more_than_64_neighbours)"""
    cfg, w, _, model = make(n=2, model=dict(g_update=g_update))
    rng = np.random.default_rng(11)
    A = 220
    degs = {0: 219, 1: 65, 7: 128, 8: 129, 9: 64, 100: 200, 219: 70}
    nb = []
    for a in range(A):
        d = degs.get(a, int(rng.integers(0, 9)))
        js = rng.choice(np.delete(np.arange(A), a), d, replace=False)
        ang = rng.uniform(0.4, 3.5, size=d)
        nb.append([[6, int(j), float(ang[k]), float(ang[k] / ang.max()), float(rng.uniform(0.9, 4.0))] for k, j in enumerate(js)])
    de, dn = so.synth_dataset(2, 3)
    de3, dn3 = np.empty(3, dtype=object), np.empty(3, dtype=object)
    de3[0], dn3[0] = de[0], dn[0]
    de3[1], dn3[1] = [[int(z) for z in rng.choice([1, 6, 7, 8], A)], 0.0], nb
    de3[2], dn3[2] = de[1], dn[1]
    inputs, _ = so.pad_batch(de3, dn3, g_update)
    names = all_names(cfg)
    got = model.predict(inputs, outputs=names)
    check_against_oracle(cfg, w, inputs, got, names)
    from scann import _hip

    rb = model.engine.upload(_hip.pack_inputs(inputs))
    assert model.engine.batch_info(rb)["big_atoms"] == 6  # (the 64-neighbour atom fits one tile)
    rb.free()


def test_outputs_at_other_widths(hip_lib):
    """64 / 4 heads / global_dim 96 / dense_out 32: the plain-fp32 kernels store the same three outputs"""
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    cfg["model"].update(local_dim=64, num_head=4, global_dim=96, dense_out=32)
    w = so.init_weights(cfg, 123, perturb=True)
    de, dn = so.synth_dataset(9, 41)
    inputs, _ = so.pad_batch(de, dn, True)
    model = HipModel(cfg, w, device=0, infer=True)
    names = all_names(cfg)
    got = model.predict(inputs, outputs=names)
    assert got[0].shape[1] == 4 and got[-2].shape[-1] == 96 and got[-1].shape == (9, 32)
    check_against_oracle(cfg, w, inputs, got, names)
    y, ga = model.predict(inputs)
    y2, ga2 = model.predict(inputs, outputs=["predict_property", "global_attention"] + names)[:2]
    assert np.array_equal(y, y2) and np.array_equal(ga, ga2)


def test_outputs_come_from_the_exact_fp32_kernels_when_the_split_range_is_left(hip_lib):
    """weights beyond the split-fp16 range (the handle runs exact-fp32 from the start), and an activation beyond it (the range guard
    fires; the forward is re-run on the exact kernels): the outputs are the exact run's, i.e. the oracle's"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    w = so.init_weights(cfg, 1234, perturb=True)
    de, dn = so.synth_dataset(9, 3)
    inputs, _ = so.pad_batch(de, dn, True)
    names = all_names(cfg)
    big = dict(w)
    big["local_attention_0/key/kernel"] = (w["local_attention_0/key/kernel"] * 4000.0).astype(np.float32)
    big["residual_norm_2/dense_1/kernel"] = (w["residual_norm_2/dense_1/kernel"] * 3000.0).astype(np.float32)
    model = HipModel(cfg, big, device=0, infer=True)
    check_against_oracle(cfg, big, inputs, model.predict(inputs, outputs=names), names, fp64_bound=True)
    bad = dict(w)
    bad["after_Lc/bias"] = (w["after_Lc/bias"] + 1.0e5).astype(np.float32)  # the activation with no LayerNorm behind it
    model = HipModel(cfg, bad, device=0, infer=True)
    assert model.engine.exact_reruns() == 0
    got = model.predict(inputs, outputs=names)
    assert model.engine.exact_reruns() == 1
    check_against_oracle(cfg, bad, inputs, got, names, fp64_bound=True)
    y_plain = model.predict(inputs)[0][:, 0]
    assert model.engine.exact_reruns() == 2
    # read before the download: scann_output_read re-runs the forward itself, the download then returns the re-run's y
    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(inputs))
    eng.set_outputs([0], after_lc=True)
    eng.forward_resident(rb, 1)
    z = eng.read_output(rb, _hip.OUT_AFTER_LC)
    assert eng.exact_reruns() == 3
    y, _ = eng.download(rb)
    eng.set_outputs()
    assert eng.exact_reruns() == 3 and np.array_equal(y, y_plain)
    assert np.array_equal(z, got[names.index("after_Lc")][inputs["atom_mask"][..., 0] != 0])
    rb.free()


def test_the_exact_rerun_writes_what_the_batch_recorded_not_what_the_handle_selects_now(hip_lib):
    """the selection belongs to the forward: cleared on the handle between the forward and its reads, the re-run of a forward whose
    range guard fired still writes the outputs the batch recorded for it (the same after_Lc/bias + 1e5 weights as above)"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    w = so.init_weights(cfg, 1234, perturb=True)
    de, dn = so.synth_dataset(9, 3)
    inputs, _ = so.pad_batch(de, dn, True)
    bad = dict(w)
    bad["after_Lc/bias"] = (w["after_Lc/bias"] + 1.0e5).astype(np.float32)
    eng = HipModel(cfg, bad, device=0, infer=True).engine
    pk = _hip.pack_inputs(inputs)
    res = []
    for clear in (False, True):
        rb = eng.upload(pk)
        eng.set_outputs([0], after_lc=True)
        eng.forward_resident(rb, 1)
        if clear:
            eng.set_outputs()
        before = eng.exact_reruns()
        a = eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 0)
        z = eng.read_output(rb, _hip.OUT_AFTER_LC)
        assert eng.exact_reruns() == before + 1
        y, ga = eng.download(rb, want_ga=True)
        assert eng.exact_reruns() == before + 1
        eng.set_outputs()
        rb.free()
        res.append((a, z, y, ga))
    for on, off in zip(*res):
        assert on.shape == off.shape and np.array_equal(on.view(np.int32), off.view(np.int32))


@pytest.mark.parametrize("g_update", [True, False], ids=["scann_plus", "base"])
def test_y_and_ga_are_bitwise_unchanged_by_outputs(hip_lib, g_update):
    from scann import _hip

    cfg, w, inputs, model = make(n=40, seed=5, model=dict(g_update=g_update))
    names = all_names(cfg)
    y0, ga0 = model.predict(inputs)
    y1, ga1 = model.predict(inputs, outputs=["predict_property", "global_attention"] + names)[:2]
    assert np.array_equal(y0, y1) and np.array_equal(ga0, ga1)
    # the resident path, the same batch: outputs off / on / off
    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(inputs))
    res = []
    for sel in (None, names, None):
        if sel:
            eng.set_outputs(range(cfg["model"]["n_attention"]), after_lc=True, bf_property=True)
        eng.forward_resident(rb, 0)
        res.append(eng.download(rb))
        eng.set_outputs()
    rb.free()
    for y, ga in res:
        assert np.array_equal(y, y0[:, 0]) and np.array_equal(ga, res[0][1])


def test_a_layer_subset_and_bad_requests(hip_lib, monkeypatch):
    from scann import _hip

    cfg, w, inputs, model = make(n=6, seed=2)
    got = model.predict(inputs, outputs=["local_attention_1"])
    assert len(got) == 1 and got[0].shape == (6, 8) + inputs["neighbors"].shape[1:]
    ref = oracle_outputs(cfg, w, inputs)
    assert rel_err(got[0], ref["local_attention_1"]) <= RTOL
    got = model.predict(inputs, outputs=["bf_property", "predict_property"])
    assert len(got) == 2 and got[0].shape == (6, 128) and np.array_equal(got[1], model.predict(inputs)[0])
    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(inputs))
    eng.set_outputs([2])
    eng.forward_resident(rb, 0)
    eng.download(rb)
    eng.set_outputs()
    assert eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 2).shape == (rb.packed.n_edge, 8)
    for what, layer in ((_hip.OUT_LOCAL_ATTENTION, 1), (_hip.OUT_AFTER_LC, 0), (_hip.OUT_BF_PROPERTY, 0)):  # not selected
        with pytest.raises(_hip.ScannHipError) as ei:
            eng.read_output(rb, what, layer)
        assert ei.value.code == -1
    eng.forward_resident(rb, 0)  # a forward with nothing selected: nothing to read
    eng.download(rb)
    with pytest.raises(_hip.ScannHipError):
        eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 2)
    rb.free()
    L = cfg["model"]["n_attention"]
    with pytest.raises(_hip.ScannHipError) as ei:
        eng.set_outputs([L])
    assert ei.value.code == -1 and "n_attention" in str(ei.value)

    def boom(*a, **k):
        raise AssertionError("launched")

    for fn in ("forward_padded", "forward", "upload", "upload_padded", "forward_resident", "set_outputs"):
        monkeypatch.setattr(eng, fn, boom)
    for bad in (["local_attention_%d" % L], ["after_lc"], ["local_attention_1", "nope"]):
        with pytest.raises(ValueError):
            model.predict(inputs, outputs=bad)


def test_chunked_and_dataset_paths_give_the_per_batch_bytes(hip_lib, monkeypatch):
    from scann.models.scann_model import HipModel
    from scann.utils import DataIterator, PackedDataset

    cfg, w, _, model = make(n=2)
    names = all_names(cfg)
    # the whole padded dataset in one call: one launch sequence, or a pipeline of chunks -- the same bytes
    de, dn = so.synth_dataset(1100, 21)
    inputs, _ = so.pad_batch(de, dn, True)
    monkeypatch.setattr(HipModel, "BIG_PREDICT", 1 << 30)
    plain = model.predict(inputs, outputs=["predict_property", "global_attention"] + names)
    monkeypatch.setattr(HipModel, "BIG_PREDICT", 1000)
    monkeypatch.setattr(HipModel, "PREDICT_CHUNK", 300)
    chunked = model.predict(inputs, outputs=["predict_property", "global_attention"] + names)
    monkeypatch.setattr(HipModel, "BIG_PREDICT", 1 << 30)
    assert len(plain) == len(chunked) == len(names) + 2
    for a, b in zip(plain, chunked):
        assert a.shape == b.shape and np.array_equal(a, b)
    # predict_dataset with fused groups against per-batch predict, structure by structure
    de, dn = so.synth_dataset(70, 41)
    it = DataIterator(de, dn, batch_size=8, g_update=True)
    pd_ = PackedDataset(de, dn, batch_size=8, g_update=True)
    ref = {n: [] for n in names}
    for i in range(len(it)):
        for n, a in zip(names, model.predict(it[i][0], outputs=names)):
            ref[n].extend(list(a))
    for data in (it, pd_):
        for group in (1, 3):
            y, ga, t, outs = model.predict_dataset(data, group=group, want_ga=True, outputs=names)
            assert len(t) == 70 and sorted(outs) == sorted(names)
            for n in names:
                assert len(outs[n]) == 70
                for s in range(70):
                    assert outs[n][s].shape == ref[n][s].shape and np.array_equal(outs[n][s], ref[n][s]), (n, s, group)
    with pytest.raises(ValueError):
        model.predict_dataset(pd_, outputs=["global_attention"])


def test_repeated_predicts_with_outputs_do_not_eat_device_memory(hip_lib):
    cfg, w, _, model = make(n=2)
    names = all_names(cfg)
    batches = []
    for n, seed in ((6, 1), (40, 2), (17, 3), (64, 4)):
        de, dn = so.synth_dataset(n, seed)
        batches.append(so.pad_batch(de, dn, True)[0])
    first = [model.predict(b, outputs=names) for b in batches]
    free0, total = model.engine.device_memory()
    for rep in range(25):
        for b, r0 in zip(batches, first):
            r = model.predict(b, outputs=names if rep % 2 == 0 else names[:1])
            assert all(np.array_equal(x, y) for x, y in zip(r, r0))
    free1, _ = model.engine.device_memory()
    assert free0 - free1 <= 32 << 20, (free0, free1)


def test_cli_writes_the_requested_outputs(hip_lib, tmp_path):
    """predict_model.py --outputs on a saved model: one pickle per output beside ga_scores_<target>.pickle, one array per structure
    in its batch's padded layout -- the arrays predict_dataset returns"""
    import yaml

    from scann.models import SCANN
    from scann.models.scann_model import save_container

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = 40
    de, dn = so.synth_dataset(n, 5)
    full = np.empty(n, dtype=object)
    for i in range(n):
        full[i] = {"Atomic": de[i][0], "Properties": {"homo": float(i)}}
    np.save(tmp_path / "data_energy.npy", full, allow_pickle=True)
    np.save(tmp_path / "data_nei.npy", dn, allow_pickle=True)
    cfg = so.default_config("qm9")
    cfg["hyper"].update(batch_size=16, scaler=False, use_ref=False, target="homo", data_energy_path=str(tmp_path / "data_energy.npy"),
                        data_nei_path=str(tmp_path / "data_nei.npy"), save_path=str(tmp_path / "run"))
    out = tmp_path / "model"
    os.makedirs(out / "models")
    yaml.safe_dump(cfg, open(out / "config.yaml", "w"))
    w = so.init_weights(cfg, 77, perturb=True)
    save_container(str(out / "models" / "model_homo.h5"), cfg, w)
    names = ["after_Lc", "local_attention_2", "bf_property"]
    r = subprocess.run([sys.executable, os.path.join(root, "predict_model.py"), str(out), "--outputs", ",".join(names)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(out / "ga_scores_homo.pickle") and os.path.exists(out / "energy_pre_homo.pickle")
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    _, _, _, ref = scann.model.predict_dataset(scann.dataIter, outputs=names)
    for nme in names:
        got = pickle.load(open(out / ("%s_homo.pickle" % nme), "rb"))
        assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, ref[nme])), nme
    sizes = [len(e[0]) for e in de]
    z = pickle.load(open(out / "after_Lc_homo.pickle", "rb"))
    assert z[0].shape == (max(sizes[:16]), 128) and not z[0][sizes[0]:].any()
    # without the flag: the CLI as before, no extra pickles
    os.remove(out / "after_Lc_homo.pickle")
    r = subprocess.run([sys.executable, os.path.join(root, "predict_model.py"), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not os.path.exists(out / "after_Lc_homo.pickle")
    # load_model_infer(path, outputs): the Keras sub-model equivalent
    sub = SCANN.load_model_infer(str(out / "models" / "model_homo.h5"), outputs=["bf_property", "predict_property"])
    inputs, _ = scann.dataIter[0]
    bf, y = sub.predict(inputs)
    assert bf.shape == (16, 128) and y.shape == (16, 1) and sub.output_names == ["bf_property", "predict_property"]
    assert np.array_equal(bf, np.stack(ref["bf_property"][:16]))

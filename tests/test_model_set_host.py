"""Host tests of model sets (no GPU): the C ABI in the header and the library, the SET kernel instantiations' resources, ModelSet's refusals
before anything is uploaded, the ensemble facade's de-normalisation and statistics, and predict_model.py's --with."""
import copy
import os
import re
import sys

import numpy as np
import pytest

import abi_checks
import scann_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("scann_models_load", "scann_models_count", "scann_forward_models", "scann_models_download")


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    from scann import _hip

    hdr = open(os.path.join(ROOT, "include", "scann_hip.h")).read()
    for n in ENTRY:
        assert re.search(r"\b%s\(" % n, hdr), n
        assert hasattr(hip_lib, n), n
        assert n in [s for s, _, _ in _hip.SYMBOLS], n


def test_set_instantiations_use_no_scratch(hip_lib):
    """atom_kernel<..., SET> (12: FFN x MODE x RT) and edge_kernel<..., SET> (8: fused first layer, plain, last layer, base branch x RT),
    the merge and readout set kernels: no scratch, within the VGPR budgets of test_default_forward_kernels_use_no_scratch"""
    from scann import _hip

    kern = abi_checks.device_kernels(_hip.LIB_PATH)
    atoms = {n: v for n, v in kern.items() if re.match(r"_ZN5scann11atom_kernelILb\dELi\dELi\dELb0ELb0ELb0ELb0ELb1EEEvNS_8AtomArgsE$", n)}
    edges = {n: v for n, v in kern.items() if re.match(r"_ZN5scann11edge_kernelILb\dELi\dELb\dELb0ELb0ELb\dELb0ELb0ELb1EEEvNS_8EdgeArgsE$", n)}
    assert len(atoms) == 12 and len(edges) == 8, (sorted(atoms), sorted(edges))
    for name, (scratch, vgpr) in {**atoms, **edges}.items():
        assert scratch == 0, (name, scratch)
        ma = re.match(r"_ZN5scann11atom_kernelILb(\d)ELi\dELi(\d)E", name)
        me = re.match(r"_ZN5scann11edge_kernelILb\dELi(\d)E", name)
        rt1 = (ma.group(2) if ma else me.group(1)) == "1"
        if not (ma and rt1 and ma.group(1) == "1"):  # (32-row ResidualNorm tiles: three workgroups per CU, as atom_kernel's launch bounds)
            assert vgpr <= (128 if rt1 else 168), (name, vgpr)
    for n in ("_ZN5scann14readout_kernelILb1EEEvNS_11ReadoutArgsE", "_ZN5scann17edge_merge_kernelILb1EEEvPKiPKfS4_S4_S4_PfPiiill"):
        assert n in kern and kern[n][0] == 0, n


class _StandInEngine:
    """records what reaches the device layer"""

    def __init__(self):
        self.loaded = None

    def models_load(self, weights, relu_out=None):
        self.loaded = (weights, relu_out)


class _StandInModel:
    def __init__(self, cfg, w):
        self.engine = _StandInEngine()
        self.made = True


def _members(K, over=None):
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 2
    out = []
    for m in range(K):
        c = copy.deepcopy(cfg)
        c["model"].update((over or {}).get(m, {}))
        out.append((c, so.init_weights(c, m)))
    return out


def test_model_set_refusals_before_any_upload():
    from scann.models import ModelSet

    made = []

    def factory(cfg, w):
        made.append(1)
        return _StandInModel(cfg, w)

    for key, val in (("local_dim", 64), ("n_attention", 3), ("g_update", False), ("use_ring", True), ("feature", "cgcnn"),
                     ("gaussian_d", 5.0), ("embedding_dim", 32)):
        mem = _members(3, {2: {key: val}})
        with pytest.raises(ValueError, match=r"member 2: model\.%s" % key):
            ModelSet(mem, engine_factory=factory)
    for K in (0, 17):
        with pytest.raises(ValueError, match="1 to 16"):
            ModelSet(_members(K), engine_factory=factory)
    mem = _members(2)
    w = dict(mem[1][1])
    w["after_Lc/kernel"] = w["after_Lc/kernel"][:, :64]
    with pytest.raises(ValueError, match="member 1: weight after_Lc/kernel"):
        ModelSet([mem[0], (mem[1][0], w)], engine_factory=factory)
    assert not made
    ms = ModelSet(_members(3), engine_factory=factory)
    assert made and len(ms.engine.loaded[0]) == 3 and ms.engine.loaded[1] == [0, 0, 0]


def test_ensemble_denormalises_each_member(monkeypatch):
    from scann.models import model_set

    mem = _members(3)
    for m, (c, _) in enumerate(mem):
        c["hyper"].update(target="homo", target_mean=str(0.5 * m), target_std=str(2.0 + m))
    raw_y = np.arange(12, dtype=np.float32).reshape(3, 4, 1) * np.float32(0.37)
    raw_ga = np.random.default_rng(0).random((3, 4, 5, 1)).astype(np.float32)
    monkeypatch.setattr(model_set.ModelSet, "predict", lambda self, inputs, batch_size=None: {"predict_property": raw_y,
                                                                                              "global_attention": raw_ga})
    ens = model_set.Ensemble(None, members=mem, engine_factory=_StandInModel)
    out = ens.predict(None)
    for m in range(3):  # predict_data's arithmetic: float32 predictions, Python-float mean / std
        assert np.array_equal(out["predict_property"][m], raw_y[m] * float(2.0 + m) + float(0.5 * m))
    yd = np.stack([raw_y[m].astype(np.float64) * (2.0 + m) + 0.5 * m for m in range(3)])
    assert np.allclose(out["mean"], yd.mean(0), rtol=0, atol=1e-12) and np.allclose(out["std"], yd.std(0, ddof=1), rtol=0, atol=1e-12)
    assert np.allclose(out["ga_std"], raw_ga.astype(np.float64).std(0, ddof=1), rtol=0, atol=1e-12)
    # mixed targets: per-target results, no ensemble statistics; an e_b member gets the mrelu head
    mem[1][0]["hyper"]["target"] = "e_b"
    ens = model_set.Ensemble(None, members=mem, engine_factory=_StandInModel)
    out = ens.predict(None)
    assert out["targets"] == ["homo", "e_b", "homo"] and "mean" not in out and "std" not in out
    assert ens.set.engine.loaded[1] == [0, 1, 0]


def test_predict_model_parser_takes_with():
    sys.path.insert(0, ROOT)
    import predict_model

    a = predict_model.parser().parse_args(["run_homo", "--with", "run_lumo,run_gap"])
    assert a.trained_model == "run_homo" and a.with_models == "run_lumo,run_gap"
    assert predict_model.parser().parse_args(["run_homo"]).with_models == ""


def _trained_dirs(tmp_path, targets, scaler=()):
    """one dataset of 30 molecules with a property per target, and a training folder per target (config.yaml + weight container)"""
    import yaml

    from scann.models.scann_model import save_container

    n = 30
    de, dn = so.synth_dataset(n, 5)
    full = np.empty(n, dtype=object)
    for i in range(n):
        full[i] = {"Atomic": de[i][0], "Properties": {"homo": 0.25 * i - 2.0, "lumo": 100.0 + 3.0 * i}}
    np.save(tmp_path / "data_energy.npy", full, allow_pickle=True)
    np.save(tmp_path / "data_nei.npy", dn, allow_pickle=True)
    dirs = []
    for k, t in enumerate(targets):
        cfg = so.default_config("qm9")
        cfg["model"]["n_attention"] = 2
        cfg["hyper"].update(batch_size=8, scaler=k in scaler, use_ref=False, target=t, data_energy_path=str(tmp_path / "data_energy.npy"),
                            data_nei_path=str(tmp_path / "data_nei.npy"), save_path=str(tmp_path / ("run%d" % k)))
        d = tmp_path / ("model%d_%s" % (k, t))
        os.makedirs(d / "models")
        yaml.safe_dump(cfg, open(d / "config.yaml", "w"))
        save_container(str(d / "models" / ("model_%s.h5" % t)), cfg, so.init_weights(cfg, k))
        dirs.append(str(d))
    return dirs, full


class _StandInSet:
    """ModelSet.predict without a device: member m predicts 10 m + (structure's atom count) / 8, scores 1 / n on real atoms"""

    def __init__(self, dirs):
        self.K = len(dirs)

    def predict(self, inputs):
        mask = inputs["atom_mask"][..., 0] != 0
        n = mask.sum(1).astype(np.float32)
        y = np.stack([(10.0 * m + n / 8).astype(np.float32) for m in range(self.K)])[..., None]
        ga = np.where(mask, 1.0 / np.maximum(n, 1)[:, None], 0.0).astype(np.float32)[None, ..., None].repeat(self.K, 0)
        return {"predict_property": y, "global_attention": ga}


def test_predict_model_with_gives_each_member_its_own_targets(tmp_path):
    """--with over K targets of one dataset: every member pairs its predictions with ITS target's values (normalised with its own
    statistics where its run sets hyper.scaler) and de-normalises with its own mean / std -- what its own run writes; no ensemble file"""
    import pickle

    sys.path.insert(0, ROOT)
    import predict_model

    dirs, full = _trained_dirs(tmp_path, ["homo", "lumo"], scaler=(1,))
    args = predict_model.parser().parse_args([dirs[0], "--with", dirs[1]])
    predict_model.main_with(args, make_set=_StandInSet)
    n_atoms = np.array([len(e["Atomic"]) for e in full], np.float32)
    homo = np.array([e["Properties"]["homo"] for e in full], np.float32)
    lumo = np.array([e["Properties"]["lumo"] for e in full], np.float32)
    mu, sd = np.mean(lumo, dtype="float32"), np.std(lumo, dtype="float32")
    y0, p0 = pickle.load(open(os.path.join(dirs[0], "energy_pre_homo.pickle"), "rb"))
    y1, p1 = pickle.load(open(os.path.join(dirs[1], "energy_pre_lumo.pickle"), "rb"))
    assert np.array_equal(np.array(y0, np.float32), homo)  # homo: unscaled, mean 0 / std 1
    assert np.array_equal(np.array(p0), n_atoms / 8)
    assert np.array_equal(np.array(y1, np.float32), ((lumo - mu) / sd).astype(np.float32))  # lumo: its own scaler
    assert np.array_equal(np.array(p1), (10.0 + n_atoms / 8).astype(np.float32) * sd + mu)
    ga = pickle.load(open(os.path.join(dirs[1], "ga_scores_lumo.pickle"), "rb"))
    assert len(ga) == len(full) and ga[0].shape == (max(n_atoms[:8]), 1)
    assert not any(f.startswith("ensemble_") for d in dirs for f in os.listdir(d))
    # one target twice: the ensemble file
    os.makedirs(tmp_path / "b")
    dirs2, _ = _trained_dirs(tmp_path / "b", ["homo", "homo"])
    predict_model.main_with(predict_model.parser().parse_args([dirs2[0], "--with", dirs2[1]]), make_set=_StandInSet)
    ens = pickle.load(open(os.path.join(dirs2[0], "ensemble_homo.pickle"), "rb"))
    assert np.allclose(ens["mean"], 5.0 + n_atoms / 8) and np.allclose(ens["std"], np.sqrt(50.0))
    # different datasets are refused
    import yaml

    c = yaml.safe_load(open(os.path.join(dirs2[1], "config.yaml")))
    c["hyper"]["batch_size"] = 16
    yaml.safe_dump(c, open(os.path.join(dirs2[1], "config.yaml"), "w"))
    with pytest.raises(SystemExit, match="batch_size"):
        predict_model.main_with(predict_model.parser().parse_args([dirs2[0], "--with", dirs2[1]]), make_set=_StandInSet)

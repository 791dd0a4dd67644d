"""Model sets: several trained models of one architecture predicted in one forward pass (scann_models_load / scann_forward_models).

A set holds K (1..16) weight sets of one configuration on one handle; every atom, edge, merge and readout launch of a set forward covers
all K members, and member m's outputs are bitwise those of a ``HipModel`` holding only member m's weights.
"""
from __future__ import annotations

import copy
import functools
import os

import numpy as np

from .. import _hip
from .scann_model import HipModel, _read_container, normalize_config

# the keys of model: that fix the architecture the members share (the widths included); hyper.target may differ (e_b: mrelu head)
ARCH_KEYS = ("n_atoms", "embedding_dim", "local_dim", "num_head", "global_dim", "dense_out", "n_attention", "gaussian_d", "g_update",
             "use_attn_norm", "use_ga_norm", "use_ring", "feature")
MAX_MEMBERS = 16


def _member_config(path):
    """(config, weights) of a model path: a weight container or a Keras .h5 (config.yaml of its training folder beside models/)"""
    import yaml

    if os.path.isdir(path):
        config = yaml.safe_load(open(os.path.join(path, "config.yaml")))
        target = config["hyper"]["target"]
        path = os.path.join(path, "models", "model_{}.h5".format(target))
        cfg, w = _read_container(path, config)
        cfg["hyper"].update({k: v for k, v in config.get("hyper", {}).items() if k != "target" or "target" not in cfg["hyper"]})
        return cfg, w
    folder = os.path.dirname(os.path.dirname(os.path.abspath(path)))
    yml = os.path.join(folder, "config.yaml")
    config = yaml.safe_load(open(yml)) if os.path.exists(yml) else None
    return _read_container(path, config)


def check_members(members):
    """[(config, weights)] -> the normalised configs; ValueError (naming the member and the key) for K outside [1, 16], an architecture
    that differs from member 0's, or weights whose names / shapes differ from member 0's"""
    K = len(members)
    if not 1 <= K <= MAX_MEMBERS:
        raise ValueError("a model set holds 1 to %d members, not %d" % (MAX_MEMBERS, K))
    cfgs = [normalize_config(copy.deepcopy(c)) for c, _ in members]
    m0 = cfgs[0]["model"]
    for i, c in enumerate(cfgs[1:], 1):
        for k in ARCH_KEYS:
            if c["model"].get(k) != m0.get(k):
                raise ValueError("member %d: model.%s is %r, member 0 has %r (a model set shares one architecture)" % (i, k, c["model"].get(k), m0.get(k)))
    shapes0 = {n: np.shape(v) for n, v in members[0][1].items()}
    for i, (_, w) in enumerate(members[1:], 1):
        shapes = {n: np.shape(v) for n, v in w.items()}
        for n in sorted(set(shapes0) | set(shapes)):
            if shapes.get(n) != shapes0.get(n):
                raise ValueError("member %d: weight %s has shape %s, member 0 has %s" % (i, n, shapes.get(n), shapes0.get(n)))
    return cfgs


class ModelSet:
    """K models of one architecture on one device.  ``members``: a list of ``(config, weights)`` or of model paths (a training folder,
    a weight container, or a Keras .h5 with its folder's config.yaml).  ``predict(inputs)`` -> {"predict_property": [K, B, 1],
    "global_attention": [K, B, M, 1]} (raw outputs; padded atoms 0)."""

    def __init__(self, members, device=None, engine_factory=None):
        members = [_member_config(m) if isinstance(m, (str, os.PathLike)) else m for m in members]
        self.configs = check_members(members)
        self.targets = [c["hyper"].get("target", "") for c in self.configs]
        factory = engine_factory or (lambda cfg, w: HipModel(cfg, w, device=device, infer=True))
        # the handle's own weights are member 0's; the set holds all K
        self.model = factory(copy.deepcopy(self.configs[0]), members[0][1])
        self.engine = self.model.engine
        self.engine.models_load([w for _, w in members], relu_out=[int(t == "e_b") for t in self.targets])
        self.n_models = len(members)

    def predict(self, inputs, batch_size=None):
        """Every member's prediction of a padded input dict or a ``PackedBatch``: {"predict_property": [K, B, 1], "global_attention":
        [K, B, M, 1]} ([K, n_atom, 1] for a PackedBatch without padding).  Inputs of more than ``batch_size`` structures (default: the
        chunk HipModel.predict uses) run in slices through HipModel's pipeline."""
        eng, K = self.engine, self.n_models
        packed_in = isinstance(inputs, _hip.PackedBatch)
        B = inputs.n_struct if packed_in else int(np.shape(inputs["neighbors"])[0])
        C = int(batch_size or HipModel.PREDICT_CHUNK)
        if C < 1:
            raise ValueError("batch_size must be >= 1")
        ys, gas = [], []

        def finish(rb, _):
            y, ga = eng.models_download(rb, want_ga=True)
            ys.append(y)
            gas.append(ga)

        if packed_in:
            jobs = ((functools.partial(eng.upload, _hip.slice_packed(inputs, s0, min(s0 + C, B))), s0) for s0 in range(0, B, C))
        else:
            jobs = ((functools.partial(self.model._upload_padded, {k: np.asarray(v)[s0:s0 + C] for k, v in inputs.items()
                                                                   if k in self.model.input_names}), s0) for s0 in range(0, B, C))
        self.model._pipeline(jobs, finish, launch=eng.forward_models)
        y = np.concatenate(ys, axis=1).reshape(K, B, 1)
        ga = np.concatenate(gas, axis=1)
        if packed_in:
            ga_out = np.stack([inputs.repad_ga(g) for g in ga]) if inputs.pad_shape is not None else ga[..., None]
        else:
            amask = np.asarray(inputs["atom_mask"]).reshape(B, -1) != 0
            ga_out = np.zeros((K,) + amask.shape, dtype=np.float32)
            ga_out[:, amask] = ga
            ga_out = ga_out[..., None]
        return {"predict_property": y, "global_attention": ga_out}


class Ensemble:
    """``SCANN.load_ensemble``: a ModelSet of trained models, each de-normalised with its own hyper.target_mean / target_std as
    predict_data does.  ``predict(inputs)`` -> {"targets": [K names], "predict_property": [K, B, 1], "global_attention": [K, B, M, 1]}
    and, when every member predicts the same target (K >= 2), "mean" / "std" (ddof 1, fp64 on the host) of the de-normalised prediction
    [B, 1] and "ga_mean" / "ga_std" of the GlobalAttention scores."""

    def __init__(self, model_dirs, device=None, engine_factory=None, members=None):
        self.set = ModelSet(members if members is not None else list(model_dirs), device=device, engine_factory=engine_factory)
        hy = [c["hyper"] for c in self.set.configs]
        self.targets = self.set.targets
        # Python floats, as SCANN keeps them: predict_data's arithmetic on the float32 predictions
        self.means = [float(h.get("target_mean", 0.0)) for h in hy]
        self.stds = [float(h.get("target_std", 1.0)) for h in hy]

    @property
    def shared_target(self):
        return len(set(self.targets)) == 1

    def predict(self, inputs, batch_size=None):
        raw = self.set.predict(inputs, batch_size=batch_size)
        y = raw["predict_property"]
        out = {"targets": list(self.targets),
               "predict_property": np.stack([y[m] * self.stds[m] + self.means[m] for m in range(len(y))]),
               "global_attention": raw["global_attention"]}
        if self.shared_target and len(y) >= 2:
            yd = np.stack([y[m].astype(np.float64) * self.stds[m] + self.means[m] for m in range(len(y))])
            ga = raw["global_attention"].astype(np.float64)
            out["mean"], out["std"] = yd.mean(axis=0), yd.std(axis=0, ddof=1)
            out["ga_mean"], out["ga_std"] = ga.mean(axis=0), ga.std(axis=0, ddof=1)
        return out

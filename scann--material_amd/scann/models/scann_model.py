"""SCANN facade on the MI355X HIP path.

Mirrors the public surface of the reference's ``scann/models/scann_model.py`` -- ``SCANN(config,
pretrained, mode)``, ``.model.predict(inputs)``, ``.prepare_dataset``, ``.evaluate``,
``.predict_data``, ``create_model`` -- with the Keras graph execution replaced by
``libscann_hip.so`` (include/scann_hip.h) through ctypes.  No TensorFlow, no PyTorch.
"""
from __future__ import annotations

import contextlib
import functools
import io
import json
import os

import numpy as np

from .. import _hip
from .latent_index import (EMBED_NEIGHBOURS, LatentClassHead, LatentClustering, LatentEmbedding, LatentHead, LatentHierarchy, LatentIndex, LatentKernelHead,
                           LatentProjection, batch_jobs, check_min_cluster_size, count_structures, density_of_sums, embed_fit_args, hierarchy_fit_args, level_dim, peaks_fit_args,
                           stop_dist2_of)

INPUT_NAMES = ["atomic", "atom_mask", "neighbors", "neighbor_mask", "neighbor_weight", "neighbor_distance"]

# keys some shipped yaml files omit (model_qm9_std.yaml / model_ptgp.yaml; train.py:37-43 injects the CLI ones)
_MODEL_DEFAULTS = dict(feature="atomic", use_ring=False, use_drop=False, g_update=False, gaussian_d=4.0,
                       use_attn_norm=True, use_ga_norm=True)
# deterministic (extension, train.py --deterministic): bit-reproducible training steps and initial weights drawn from hyper.seed
# freeze / lr_scale / reset (extension, train.py --freeze / --lr-scale / --reset; scann/models/finetune.py): fine-tuning -- patterns over
# tensor names that freeze tensors, scale their learning rate, or draw them afresh after a pretrained checkpoint is loaded; None: absent
_HYPER_DEFAULTS = dict(scaler=False, scheduler="cosine", use_ref=False, target="", pretrained="", deterministic=False,
                       freeze=None, lr_scale=None, reset=None)


def normalize_config(config):
    """Fill the keys the reference reads but some of its yaml files lack (deliberate deviation: the
    reference raises KeyError there)."""
    config.setdefault("model", {})
    config.setdefault("hyper", {})
    for k, v in _MODEL_DEFAULTS.items():
        config["model"].setdefault(k, v)
    for k, v in _HYPER_DEFAULTS.items():
        config["hyper"].setdefault(k, v)
    return config


def config_struct(config):
    m = config["model"]
    if m["feature"] not in ("atomic", "cgcnn"):
        raise ValueError("model.feature must be 'atomic' or 'cgcnn'")
    return _hip.Config(
        n_atoms=int(m["n_atoms"]), embedding_dim=int(m["embedding_dim"]), local_dim=int(m["local_dim"]),
        num_head=int(m["num_head"]), n_attention=int(m["n_attention"]), global_dim=int(m["global_dim"]),
        dense_out=int(m["dense_out"]), n_gauss=20, gaussian_d=float(m["gaussian_d"]),
        g_update=int(bool(m["g_update"])), use_attn_norm=int(bool(m["use_attn_norm"])),
        use_ga_norm=int(bool(m["use_ga_norm"])), use_ring=int(bool(m["use_ring"])),
        feature_cgcnn=int(m["feature"] == "cgcnn"),
        relu_out=int(config["hyper"].get("target") == "e_b"),  # scann_model.py:446
    )


def keras_default_init(specs, seed=None):
    """Keras default initialisers for a fresh model (what create_model yields before training):
    Dense kernels Glorot-uniform, biases 0, Embedding U(-0.05, 0.05), LayerNorm gamma 1 / beta 0."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in specs:
        leaf = name.rsplit("/", 1)[1]
        if leaf == "kernel":
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            t = rng.uniform(-lim, lim, size=shape)
        elif leaf == "embeddings":
            t = rng.uniform(-0.05, 0.05, size=shape)
        elif leaf == "gamma":
            t = np.ones(shape)
        else:
            t = np.zeros(shape)
        w[name] = np.ascontiguousarray(t, dtype=np.float32)
    return w


def save_container(path, config, weights):
    """Write the weight container ATOMICALLY: the bytes go to a temporary file in the same directory, which then replaces
    ``path`` (os.replace).  A reader -- another rank loading the best checkpoint, a monitoring script -- sees the previous
    complete file or the new complete file, never a partial one."""
    buf = io.BytesIO()
    np.savez(buf, __config__=np.array(json.dumps(config)), **weights)
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    tmp = os.path.join(folder, ".%s.%d.tmp" % (os.path.basename(path), os.getpid()))
    try:
        with open(tmp, "wb") as f:
            f.write(buf.getvalue())
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)


OUTPUT_NAMES = ("predict_property", "global_attention", "after_Lc", "bf_property")  # + local_attention_<k>


def _output_selection(names, n_attention):
    """Validate a list of output names (the reference's Keras layer names): ``predict_property``, ``global_attention``,
    ``local_attention_<k>`` (k < n_attention), ``after_Lc``, ``bf_property``.  -> (names, attention layers, after_Lc?, bf_property?);
    ValueError before anything runs."""
    if isinstance(names, str):
        names = [names]
    names = list(names)
    layers = []
    for n in names:
        if not isinstance(n, str):
            raise ValueError("output names are strings, got %r" % (n,))
        if n.startswith("local_attention_"):
            k = n[len("local_attention_"):]
            if not k.isdigit() or str(int(k)) != k:
                raise ValueError("unknown output %r" % n)
            if int(k) >= n_attention:
                raise ValueError("%s: the model has %d local-attention layers (local_attention_0 .. local_attention_%d)" % (
                    n, n_attention, n_attention - 1))
            layers.append(int(k))
        elif n not in OUTPUT_NAMES:
            raise ValueError("unknown output %r (known: %s, local_attention_<k>)" % (n, ", ".join(OUTPUT_NAMES)))
    return names, sorted(set(layers)), "after_Lc" in names, "bf_property" in names


# -- the steps the analysis methods of HipModel share: a new analysis uses these rather than a neighbour's lines --

def _expect(value, cls, noun):
    """ValueError unless ``value`` is the artefact a method takes"""
    if not isinstance(value, cls):
        raise ValueError("%s must be a %s, got %r" % (noun, cls.__name__, type(value).__name__))


def _level_of(data, level):
    """The level in force: a ``LatentIndex``'s own, ``level`` for data that is yet to be indexed"""
    return data.level if isinstance(data, LatentIndex) else level


def _flat_per_structure(values, level, noun, dtype=None):
    """Atom-level targets or labels given as one array per structure -> one array in packed order (anything else: as it is).  With a
    ``dtype`` every structure's array is rows [n, ...] of that type, without one a vector."""
    if level == "atom" and isinstance(values, (list, tuple)) and len(values) and np.ndim(values[0]) >= 1:
        try:
            if dtype is None:
                return np.concatenate([np.asarray(x).reshape(-1) for x in values])
            return np.concatenate([np.asarray(x, dtype=dtype).reshape(len(x), -1) for x in values])
        except (TypeError, ValueError):
            raise ValueError("%s must be a flat array in packed order or one array per structure" % noun) from None
    return values


def _exclude_ids_arg(inputs, exclude_ids):
    """``exclude_ids`` as int64 [B], one per structure of ``inputs`` (None stays None); ValueError for another count"""
    if exclude_ids is None:
        return None
    B = count_structures(inputs)
    qid = np.ascontiguousarray(exclude_ids, dtype=np.int64).reshape(-1)
    if qid.shape[0] != B:
        raise ValueError("exclude_ids: %d structures need %d ids, got %d" % (B, B, qid.shape[0]))
    return qid


def _repad(out, inputs, level, fills, dtypes=None):
    """The per-atom entries of ``out`` -- ``fills``: {name: value at padded atoms} -- from packed [n_atom, ...] to [B, M, ...] when the
    rows are atoms and ``inputs`` is a padded dict; a ``PackedBatch`` keeps them packed.  ``dtypes``: {name: dtype} for entries that
    are not to come back as fp32 (``_hip.repad_atoms``).  Returns ``out``."""
    if level == "atom" and not isinstance(inputs, _hip.PackedBatch):
        for n, fill in fills.items():
            out[n] = _hip.repad_atoms(out[n], inputs["atom_mask"], fill, dtype=(dtypes or {}).get(n))
    return out



class HipModel:
    """Stand-in for the ``tf.keras.Model`` that ``create_model`` returns (scann_model.py:449):
    ``predict`` runs the whole forward graph on the GPU."""

    def __init__(self, config, weights=None, device=None, infer=False, seed=None, outputs=None, deterministic=None):
        self.config = normalize_config(config)
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("SCANN_DEVICE") is None \
                else int(os.environ["SCANN_DEVICE"])
        self.engine = _hip.Engine(config_struct(self.config), device)
        self.infer = infer  # True: outputs [y, global_attention scores] (scann_model.py:81-83)
        self.input_names = list(INPUT_NAMES) + (["ring_aromatic"] if self.config["model"]["use_ring"] else [])
        self.output_names = ["predict_property"] + (["global_attention"] if infer else [])
        self.outputs = None  # a list of output names: what predict returns when its call names none (load_model_infer(path, outputs))
        if outputs is not None:
            self.outputs = _output_selection(outputs, int(self.config["model"]["n_attention"]))[0]
            self.output_names = list(self.outputs)
        self._weights = None
        self.set_weights(weights if weights is not None else keras_default_init(self.engine.weight_specs(), seed))
        # deterministic training mode (scann_set_deterministic): every gradient of a step summed in a fixed order
        self.deterministic = bool(self.config["hyper"]["deterministic"] if deterministic is None else deterministic)
        if self.deterministic:
            self.engine.set_deterministic(True)

    # -- weights ---------------------------------------------------------------------------------
    def set_weights(self, weights):
        self.engine.load_weights(weights)
        self._weights = {n: np.array(weights[n], dtype=np.float32) for n, _ in self.engine.weight_specs()}

    def get_weights(self):
        return dict(self._weights)

    def count_params(self):
        return int(sum(v.size for v in self._weights.values()))

    def save(self, path):
        """Weight container: a zip (npz) of the named fp32 tensors plus the yaml config as JSON.
        Takes the place of the Keras full-model HDF5 (scann_model.py:166-177)."""
        save_container(path, self.config, self._weights)

    # -- inference ---------------------------------------------------------------------------------
    def predict(self, inputs, batch_size=None, verbose=0, outputs=None, **_):
        """``model.predict(inputs)`` (scann_model.py:266,316): ``[B,1]`` or, in infer mode,
        ``[[B,1], [B,M,1]]``.

        ``outputs`` (a list of the reference's layer names; what a Keras sub-model of the graph would return): a list in that order.
        ``predict_property`` [B,1] and ``global_attention`` [B,M,1] as above; ``local_attention_<k>`` -- layer k's attention weights
        (attention.py:189) -- [B, num_head, M, N]; ``after_Lc`` [B, M, global_dim] (zero rows for padded atoms); ``bf_property``
        [B, dense_out].  For a ``PackedBatch`` the per-edge / per-atom outputs stay packed: [n_edge, num_head], [n_atom, global_dim].
        Unknown names and layers >= n_attention raise ValueError before anything runs."""
        m = self.config["model"]
        if outputs is None and self.outputs is not None:
            outputs = self.outputs
        sel = None if outputs is None else _output_selection(outputs, int(m["n_attention"]))
        if not isinstance(inputs, _hip.PackedBatch):
            nb = np.shape(inputs["neighbors"])
            slots = int(nb[0]) * int(nb[1]) * max(1, int(nb[2]))  # padded neighbour slots >= edges; >= atoms
            if nb[0] >= self.BIG_PREDICT or (slots > self.BIG_SLOTS and nb[0] > 1):
                return self._predict_chunked(inputs, sel)
        if sel is not None:
            return self._predict_outputs(inputs, sel)
        if not isinstance(inputs, _hip.PackedBatch) and m["feature"] == "atomic" and not m["use_ring"]:
            y, ga = self.engine.forward_padded(inputs, want_ga=self.infer)  # native CSR packing
            return [y.reshape(-1, 1), ga] if self.infer else y.reshape(-1, 1)
        packed = inputs if isinstance(inputs, _hip.PackedBatch) else _hip.pack_inputs(inputs)
        y, ga = self.engine.forward(packed, want_ga=self.infer)
        y = y.reshape(-1, 1)
        if self.infer:
            return [y, packed.repad_ga(ga)]
        return y

    __call__ = predict

    GRAD_INPUTS = ("neighbor_distance", "neighbor_weight", "ring_aromatic", "atomic")

    def input_gradients(self, inputs, wrt=("neighbor_distance", "neighbor_weight"), batch_size=None):
        """Gradients of each structure's own raw prediction y_s (``predict_property`` before any target de-normalisation) with
        respect to its inputs, under inference semantics (no Dropout) -- what ``tf.GradientTape`` over ``model(inputs)`` gives for the
        reference's graph, per structure.  ``wrt``: any of ``neighbor_distance``, ``neighbor_weight``, ``ring_aromatic`` (use_ring) and
        ``atomic`` (feature cgcnn: the [.., 92] features).  Returns {name: gradient} plus ``predict_property`` [B, 1].  A padded dict
        gives [B, M, N] / [B, M, 2] / [B, M, 92], 0 in masked slots and padded atoms; a ``PackedBatch`` gives packed [n_edge] /
        [n_atom, 2] / [n_atom, 92].  Inputs are run ``batch_size`` structures at a time (default: hyper.batch_size) and the results
        concatenated.  Unknown names, or names the configuration has no such input for, raise ValueError before anything runs."""
        m = self.config["model"]
        wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
        for n in wrt:
            if n not in self.GRAD_INPUTS:
                raise ValueError("no gradient with respect to %r (one of %s)" % (n, ", ".join(self.GRAD_INPUTS)))
            if n == "ring_aromatic" and not m["use_ring"]:
                raise ValueError("ring_aromatic: the model has no ring input (use_ring is off)")
            if n == "atomic" and m["feature"] != "cgcnn":
                raise ValueError("atomic: gradients exist for the cgcnn features only (the atomic numbers are integers)")
        flags = dict(distance="neighbor_distance" in wrt, weight="neighbor_weight" in wrt, ring="ring_aromatic" in wrt,
                     cgcnn="atomic" in wrt)
        eng = self.engine
        # (batch_size 0 has always meant the default here; padded chunks are packed on the host, whose packer names a bad input at once)
        parts = self._run_chunks(inputs, batch_size or None, lambda rb, s0, s1: eng.input_grads(rb, **flags), host_pack=True)
        out = {n: np.concatenate([p[n] for p in parts]) for n in wrt}
        if not isinstance(inputs, _hip.PackedBatch):  # (chunks are consecutive structures: their packed results, concatenated, are the input's)
            amask, nmask = inputs["atom_mask"], inputs["neighbor_mask"]
            for n in wrt:
                out[n] = _hip.repad_atoms(out[n], amask) if n in ("ring_aromatic", "atomic") else _hip.repad_edges(out[n], amask, nmask)
        out["predict_property"] = np.concatenate([p["y"] for p in parts]).reshape(-1, 1)
        return out

    def atom_contributions(self, inputs, mode="leave_one_out", batch_size=None):
        """How much of each structure's raw prediction hangs on each atom's local-structure representation: the prediction with atoms
        left out of the GlobalAttention pooling and everything upstream unchanged -- the reference's ``model.predict`` with ``atom_mask``
        zeroed on those atoms, which feeds nothing but the pooling (scann_model.py:329-447) -- for all kept sets of one ``mode`` from one
        forward.  Atoms are ranked by the GlobalAttention scores of the unablated forward, descending, ties by ascending index.
        ``leave_one_out``: entry r = all atoms but r; ``deletion``: entry k - 1 = all but the k highest-ranked; ``insertion``: entry
        k - 1 = the k highest-ranked only.  ``inputs``: a padded dict, run ``batch_size`` structures at a time (default:
        hyper.batch_size).  Returns {"y": [B, 1], "global_attention": [B, M, 1], "ablated": [B, M, 1] (entry e at the padded position
        of the structure's e-th real atom, 0 at padding), "order": [B, M] int32 (padded-array atom index by rank, -1 at padding)} and,
        for ``leave_one_out``, "contribution": [B, M, 1] = y - ablated in fp32.  With use_ga_norm a pooling over one atom or none is the
        reference's 0 / 0 = NaN.  A bad mode or batch_size raises ValueError before anything is uploaded."""
        if mode not in _hip.ABLATE_MODES:
            raise ValueError("mode must be one of %s, got %r" % (", ".join(_hip.ABLATE_MODES), mode))
        eng = self.engine
        B = int(np.shape(inputs["neighbors"])[0])
        amask = np.asarray(inputs["atom_mask"]).reshape(B, -1) != 0
        parts = self._run_chunks(inputs, batch_size, lambda rb, s0, s1: eng.ablate_pooling(rb, mode))
        cat = {k: np.concatenate([p[k] for p in parts]) for k in ("y", "ga", "ablated", "order")}
        y = cat["y"].reshape(-1, 1)
        out = {"y": y, "global_attention": _hip.repad_atoms(cat["ga"], amask)[..., None], "ablated": _hip.repad_atoms(cat["ablated"], amask)[..., None]}
        # rank -> padded position: the structure's e-th real atom sits at the e-th set position of its mask row
        order = np.full(amask.shape, -1, dtype=np.int32)
        rows, cols = np.nonzero(amask)
        first = np.concatenate([[0], np.cumsum(amask.sum(1))])[rows]  # packed offset of each real atom's structure
        order[rows, cols] = cols[first + cat["order"]]
        out["order"] = order
        if mode == "leave_one_out":
            out["contribution"] = np.where(amask[..., None], y[:, None, :] - out["ablated"], np.float32(0)).astype(np.float32)
        return out

    def atom_shapley(self, inputs, permutations=64, seed=0, keys=None, batch_size=None):
        """Shapley values of a structure's atoms for the GlobalAttention pooling, sampled on the GPU: the raw prediction split fairly
        among the atoms.  The game: v(S) is the prediction with the atoms outside S left out of the pooling and everything upstream
        unchanged (``atom_contributions``' kept sets); an atom's Shapley value is its marginal v(S + i) - v(S) averaged over the orders in
        which atoms can be added, here over ``permutations`` random orders per structure, all from one forward.  For |S| <= 1, where the
        reference's use_ga_norm arithmetic is 0 / 0, the game uses that of use_ga_norm = false (the continuous extension: one kept atom
        pools to its own row, none to 0), so ``baseline`` = v(nothing) is the head on a zero representation.  Efficiency: a structure's
        values sum to ``full - baseline``, ``full`` being the mean of v(all atoms) over the walks (y in another summation order).
        ``stderr``: the standard error of each value over the walks (NaN for one walk).  The walks of a structure depend on ``seed``,
        its key and its atom count only (``keys``: one integer per structure, default its position in ``inputs``), so ``batch_size``
        changes no bit.  ``inputs``: a padded dict.  Returns float64 {"y": [B, 1], "global_attention": [B, M, 1], "shapley": [B, M, 1],
        "stderr": [B, M, 1], "baseline": [B, 1], "full": [B, 1]}, 0 at padding.  A one-atom structure under use_ga_norm has y = NaN, and
        NaN values.  Bad arguments raise ValueError before anything is uploaded."""
        try:
            P, sd = int(permutations), int(seed)
        except (TypeError, ValueError):
            raise ValueError("permutations and seed must be integers, got %r and %r" % (permutations, seed))
        if P != permutations or P < 1:
            raise ValueError("permutations must be an integer >= 1, got %r" % (permutations,))
        if sd != seed or sd < 0:
            raise ValueError("seed must be a non-negative integer, got %r" % (seed,))
        B = int(np.shape(inputs["neighbors"])[0])
        if keys is None:
            keys = np.arange(B, dtype=np.uint64)
        else:
            keys = np.asarray(keys).reshape(-1)
            if keys.shape[0] != B:
                raise ValueError("keys: %d values for %d structures" % (keys.shape[0], B))
            if not np.issubdtype(keys.dtype, np.integer) or (keys.size and int(keys.min()) < 0):
                raise ValueError("keys must be non-negative integers")
            keys = keys.astype(np.uint64)
        eng = self.engine
        amask = np.asarray(inputs["atom_mask"]).reshape(B, -1) != 0
        parts = self._run_chunks(inputs, batch_size, lambda rb, s0, s1: eng.shapley(rb, P, seed=sd, keys=keys[s0:s1]))
        cat = {k: np.concatenate([p[k] for p in parts]) for k in ("y", "ga", "shapley", "stderr", "baseline", "full")}
        out = {k: cat[k].astype(np.float64).reshape(-1, 1) for k in ("y", "baseline", "full")}
        for name, k in (("global_attention", "ga"), ("shapley", "shapley"), ("stderr", "stderr")):
            out[name] = _hip.repad_atoms(cat[k], amask, dtype=np.float64)[..., None]
        return out

    def attention_rollout(self, inputs, residual=0.5, head=None, depth=None, matrix=True, batch_size=None):
        """Which atoms a structure's prediction traces back to through the LocalAttention layers: attention rollout (Abnar & Zuidema
        2020).  A GlobalAttention score belongs to an atom's local structure after n_attention rounds of message passing; the rollout
        multiplies the layers' attention maps through -- per layer the head-averaged map (``head`` None; or head k alone) mixed with
        ``residual`` of the identity for the skip connection, an atom without neighbours keeping its row -- for the first ``depth``
        layers (None: all).  ``rollout[i, j]``: the share of atom i's final representation that comes from atom j (rows sum to 1);
        ``atom_attribution[j] = sum_i global_attention[i] * rollout[i, j]`` sums to 1 over a structure.  All from one forward, composed
        on the GPU.  A padded dict gives {"predict_property": [B, 1], "global_attention": [B, M, 1], "atom_attribution": [B, M, 1],
        "rollout": [B, M, M]} (row / column at the padded position of the atom, 0 at padding; ``matrix=False``: no "rollout"); a
        ``PackedBatch`` gives the packed [n_atom] arrays, "rollout" [sum n^2] (the structures' n x n row-major blocks) and
        "rollout_offset" [n_struct + 1].  Raw y.  Inputs run ``batch_size`` structures at a time (default: hyper.batch_size).  At most
        _hip.ROLLOUT_MAX_ATOMS atoms per structure.  Bad arguments raise ValueError before anything is uploaded."""
        m = self.config["model"]
        args = _hip.check_rollout_args(residual, head, depth, int(m["num_head"]), int(m["n_attention"]))
        eng = self.engine
        parts = self._run_chunks(inputs, batch_size, lambda rb, s0, s1: eng.attention_rollout(
            rb, args[0], None if args[1] < 0 else args[1], args[2] or None, matrix=bool(matrix)))
        keys = ("y", "ga", "attribution") + (("rollout",) if matrix else ())
        cat = {k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, np.float32) for k in keys}
        sq = np.concatenate([np.diff(p["rollout_offset"]) for p in parts]) if parts else np.zeros(0, np.int64)  # n^2 per structure
        offset = np.concatenate([[0], np.cumsum(sq)]).astype(np.int64)
        y = cat["y"].reshape(-1, 1)
        if isinstance(inputs, _hip.PackedBatch):
            out = {"predict_property": y, "global_attention": cat["ga"], "atom_attribution": cat["attribution"], "rollout_offset": offset}
            if matrix:
                out["rollout"] = cat["rollout"]
            return out
        amask = np.asarray(inputs["atom_mask"])
        amask = amask.reshape(amask.shape[:2]) != 0
        out = {"predict_property": y, "global_attention": _hip.repad_atoms(cat["ga"], amask)[..., None],
               "atom_attribution": _hip.repad_atoms(cat["attribution"], amask)[..., None]}
        if matrix:
            B, M = amask.shape
            R = np.zeros((B, M, M), dtype=np.float32)
            for b in range(B):
                pos = np.nonzero(amask[b])[0]
                R[b][np.ix_(pos, pos)] = cat["rollout"][offset[b]:offset[b + 1]].reshape(len(pos), len(pos))
            out["rollout"] = R
        return out

    def build_index(self, data, level="structure", ids=None, batch_size=None, cells=None):
        """A ``LatentIndex`` of ``data`` on this model's GPU: one ``bf_property`` row per structure (``level`` "structure") or one
        ``after_Lc`` row per real atom ("atom"), computed batch by batch and kept on the device.  ``data``: a padded dict, a
        ``PackedBatch`` or a dataset as ``predict_dataset`` takes it; ``ids``: one per structure (default 0 .. n-1 in input order).  A bad
        level or batch_size raises ValueError before anything is uploaded.  ``cells`` ("auto" or 1 .. 1024; default None: none): partition the
        finished index (``LatentIndex.partition``), so that ``nearest``, ``place``, ``attach`` and ``select_diverse`` skip cells out of
        reach; their answers do not change."""
        level_dim(self.config, level)
        self._batch_size(batch_size)
        if cells is not None and cells != "auto":
            _hip.check_cells_args(cells, 0)
        index = LatentIndex(self, level).add(data, ids=ids, batch_size=batch_size)
        if cells is not None and len(index):
            index.partition(cells)
        return index

    def nearest(self, inputs, index, k=5, exclude_ids=None, batch_size=None):
        """The ``k`` nearest rows of a ``LatentIndex`` for every structure (or, for an atom-level index, every atom) of ``inputs``, by
        Euclidean distance between the learned representations, searched on the GPU right behind the forward.  Rows are ranked by
        (distance, position in the index): the result depends on the query and the index only.  ``exclude_ids`` [B]: rows whose id
        equals the structure's are skipped (leave-one-out).  A padded dict gives {"predict_property": [B, 1], "distance": [B, k] fp32,
        "neighbor_id": [B, k] int64, "latent_distance": [B, 1]} -- the mean of the k distances, ``inf`` if fewer than k rows qualify
        (those places: distance inf, id -1) -- and at atom level [B, M, k] / [B, M, 1] arrays plus "neighbor_atom" [B, M, k], with
        0 / -1 at padded atoms; a ``PackedBatch`` gives packed [n_atom, k] arrays.  Raw y.  ``batch_size`` structures at a time (default:
        hyper.batch_size).  A k outside 1 .. 32, an index of another model or width, or a bad batch_size raise ValueError before anything
        is uploaded."""
        k = _hip.check_knn_k(k)
        _expect(index, LatentIndex, "index")
        index.check_model(self)
        qid = _exclude_ids_arg(inputs, exclude_ids)
        eng, lvl = self.engine, _hip.KNN_LEVELS[index.level]
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.index_query_batch(
            index._ix, rb, lvl, k, None if qid is None else qid[s0:s1]),
            {"y": np.zeros(0, np.float32), "dist2": np.zeros((0, k), np.float32), "id": np.zeros((0, k), np.int64), "atom": np.zeros((0, k), np.int32)})
        dist = np.sqrt(cat["dist2"])  # correctly rounded on the host: no device square root enters the definition
        mean = np.zeros(dist.shape[0], dtype=np.float32)
        for j in range(k):  # fp32, places in order
            mean = mean + dist[:, j]
        mean = (mean / np.float32(k)).astype(np.float32)[:, None]
        out = {"predict_property": cat["y"].reshape(-1, 1), "distance": dist, "neighbor_id": cat["id"], "latent_distance": mean}
        if index.level == "atom":
            out["neighbor_atom"] = cat["atom"]
        return _repad(out, inputs, index.level, {"distance": 0, "latent_distance": 0, "neighbor_id": -1, "neighbor_atom": -1})

    def within(self, inputs, index, radius, exclude_ids=None, batch_size=None, max_pairs=1 << 24, count_only=False):
        """Which rows of a ``LatentIndex`` lie within Euclidean distance ``radius`` of every structure (or, for an atom-level index,
        every atom) of ``inputs``: the exact radius search on the GPU right behind the forward (scann_index_within_batch).  This is the
        leakage check of a benchmark -- ``count > 0`` names the test structures that have a training twin, and the lists say which
        training structure -- and the ball count of a prediction.  ``exclude_ids`` [B]: rows whose id equals the structure's are
        skipped.  Returns {"predict_property": [B, 1] (raw y), "count": int64 [B], or [B, M] at atom level with 0 at padded atoms (a
        ``PackedBatch`` gives the packed [n_atom]), "first": int64 [nq + 1] over the nq query rows in packed order, "position" int32,
        "neighbor_id" int64, "neighbor_atom" int32, "dist2", "distance" fp32 [total]}: the hits of query row i are entries first[i] ..
        first[i + 1] - 1 in the order (distance, position); ``count_only`` leaves the lists out.  ``LatentIndex.within`` defines the
        radius.  More than ``max_pairs`` hits in all, an index of another model or width, or bad arguments raise ValueError before
        anything is uploaded."""
        from .latent_index import radius2_of

        r2 = radius2_of(radius)
        _, max_pairs, _ = _hip.check_within_args(r2, max_pairs)
        _expect(index, LatentIndex, "index")
        index.check_model(self)
        qid = _exclude_ids_arg(inputs, exclude_ids)
        eng, lvl, found = self.engine, _hip.KNN_LEVELS[index.level], [0]

        def call(rb, s0, s1):
            r = eng.index_within_batch(index._ix, rb, lvl, r2, None if qid is None else qid[s0:s1], max_pairs=max_pairs - found[0],
                                       count_only=count_only)
            found[0] += 0 if count_only else r["total"]
            return r

        names = {"y": np.float32, "count": np.int64} if count_only else {
            "y": np.float32, "count": np.int64, "position": np.int32, "id": np.int64, "atom": np.int32, "dist2": np.float32}
        cat = self._run_cat(inputs, batch_size, call, {n: np.zeros(0, t) for n, t in names.items()})
        out = {"predict_property": cat["y"].reshape(-1, 1), "count": cat["count"],
               "first": np.concatenate([[0], np.cumsum(cat["count"])]).astype(np.int64)}
        if not count_only:
            out.update({"position": cat["position"], "neighbor_id": cat["id"], "neighbor_atom": cat["atom"], "dist2": cat["dist2"],
                        "distance": np.sqrt(cat["dist2"])})
        return _repad(out, inputs, index.level, {"count": 0}, {"count": np.int64})

    def duplicates(self, data, radius, level="structure", batch_size=None, max_pairs=1 << 24):
        """The near-duplicate groups of ``data`` in the model's latent space: the same crystal entered twice, conformers the model cannot
        tell apart (``LatentIndex.duplicates``, whose dict this returns; ``keep`` is the dedup mask).  ``data`` is a ``LatentIndex`` (its
        level counts, not ``level``) or data as ``build_index`` takes it, which is indexed for the call and freed afterwards.  Bad
        arguments raise ValueError before anything is uploaded."""
        from .latent_index import radius2_of

        level_dim(self.config, _level_of(data, level))
        _hip.check_within_args(radius2_of(radius), max_pairs)
        self._batch_size(batch_size)
        with self._indexed(data, level, batch_size=batch_size) as index:
            return index.duplicates(radius, max_pairs=max_pairs)

    def match_structures(self, inputs, index, k=5, measure="chamfer", exclude_ids=None, batch_size=None):
        """The ``k`` structures of an atom-level ``LatentIndex`` that are made of the same local structures as each structure of
        ``inputs``: the two are compared as sets of ``after_Lc`` rows on the GPU right behind the forward (scann_index_match_batch).
        With f_i the squared distance of query atom i to its nearest atom of the indexed structure and g_j the same from the indexed
        structure's atom j, ``measure`` "chamfer" scores mean f + mean g, "hausdorff" max(max f, max g), and "cover" mean f alone
        (does every local structure of the query occur there?).  Structures are ranked by (score, position in the index): the result
        depends on the query and the index only, bit for bit.  ``exclude_ids`` [B]: indexed structures whose id equals the
        structure's are skipped (leave-one-out).  Returns {"predict_property": [B, 1], "distance": [B, k] fp32 -- the square root of
        the score --, "neighbor_id": [B, k] int64, "neighbor_size": [B, k] int32 (atoms of the neighbour), "parts": [B, k, 4] (mean f,
        mean g, max f, max g, squared), "matched_atom": [B, M, k] int32 -- the atom of the neighbour that query atom i matches, its index within that
        structure -- and "matched_distance": [B, M, k] fp32 = sqrt(f_i)}, -1 / 0 at padded atoms; a ``PackedBatch`` gives packed
        [n_atom, k] arrays.  Places without a neighbour hold distance inf, id -1, size 0, matched_atom -1.  Raw y.  ``batch_size``
        structures at a time (default: hyper.batch_size).  A structure-level index, an index of another model, a bad k, measure,
        batch_size or exclude_ids length, or a structure of more than _hip.MATCH_MAX_ATOMS atoms raise ValueError before anything is
        uploaded."""
        k, ms = _hip.check_knn_k(k), _hip.check_match_measure(measure)
        self._atom_query(inputs, index, "match_structures", _hip.MATCH_MAX_ATOMS, batch_size)
        qid = _exclude_ids_arg(inputs, exclude_ids)
        eng = self.engine
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.index_match_batch(
            index._ix, rb, k, ms, None if qid is None else qid[s0:s1]),
            {"y": np.zeros(0, np.float32), "score": np.zeros((0, k), np.float32), "id": np.zeros((0, k), np.int64),
             "size": np.zeros((0, k), np.int32), "parts": np.zeros((0, k, 4), np.float32),
             "match_position": np.zeros((0, k), np.int32), "match_dist2": np.zeros((0, k), np.float32)})
        _, atoms = eng.index_names(index._ix)  # (host copies: the rows stay on the device)
        pos = cat["match_position"]
        matched = np.where(pos >= 0, atoms[np.maximum(pos, 0)] if len(atoms) else -1, -1).astype(np.int32)
        out = {"predict_property": cat["y"].reshape(-1, 1), "distance": np.sqrt(cat["score"]),  # (correctly rounded on the host, as nearest)
               "neighbor_id": cat["id"], "neighbor_size": cat["size"], "parts": cat["parts"], "matched_atom": matched,
               "matched_distance": np.sqrt(cat["match_dist2"])}
        return _repad(out, inputs, "atom", {"matched_atom": -1, "matched_distance": 0})

    def _atom_query(self, inputs, index, who, most_atoms, batch_size):
        """What the atom-by-atom comparisons refuse before anything is uploaded: an ``index`` that is no atom-level ``LatentIndex`` of
        this model, a bad batch_size, a structure of more than ``most_atoms`` atoms.  Returns the atoms per structure."""
        _expect(index, LatentIndex, "index")
        index.check_model(self)
        if index.level != "atom":
            raise ValueError("%s compares structures atom by atom: it needs an atom-level index, got a %s-level one" % (who, index.level))
        self._batch_size(batch_size)
        return self._atoms_per_structure(inputs, most_atoms)

    @staticmethod
    def _atoms_per_structure(inputs, most_atoms):
        """Atoms of every structure of ``inputs``; ValueError naming the first with more than ``most_atoms``"""
        is_packed = isinstance(inputs, _hip.PackedBatch)
        n_at = np.diff(inputs.mol_offset) if is_packed else (np.asarray(inputs["atom_mask"]).reshape(count_structures(inputs), -1) != 0).sum(1)
        big = np.nonzero(n_at > most_atoms)[0]
        if big.size:
            raise ValueError("structure %d has %d atoms, more than the %d a query structure may have" % (big[0], int(n_at[big[0]]), most_atoms))
        return n_at

    def pair_structures(self, inputs, index, k=5, shortlist=32, measure="chamfer", exclude_ids=None, batch_size=None):
        """``match_structures`` with a true atom map: the ``k`` structures of an atom-level ``LatentIndex`` nearest to each structure of
        ``inputs`` under the one-to-one pairing of their atoms -- the linear assignment problem over the squared distances of the
        ``after_Lc`` rows, solved exactly on the GPU right behind the forward (scann_index_pairing_batch; the definition is in
        include/scann_hip.h).  Every query atom gets its own atom of the neighbour, so the map lines two structures up atom by atom and
        the score counts: structures made of the same local structures in different numbers are not at distance 0.  The candidates are
        the ``shortlist`` nearest structures under ``measure`` (``match_structures``' measures; ``exclude_ids`` applies there), reranked
        by (pairing score, position in the index); the result depends on the query, the index and (k, shortlist, measure) only.
        Returns {"predict_property": [B, 1], "distance": [B, k] fp32 -- the square root of the pairing score, the mean squared distance
        over max(n, m) pairs with a surplus atom charged its nearest partner --, "neighbor_id": [B, k] int64, "neighbor_size": [B, k],
        "shortlist_distance": [B, k] (the neighbour's distance under ``measure``), "shortlist_place": [B, k] (its place in the
        shortlist), "paired_atom": [B, M, k] int32 -- the atom's partner, its index within the neighbour, -1 where the atom is surplus
        or at padding --, "paired_distance": [B, M, k] fp32 (for a surplus atom: to its nearest atom), "surplus": [B, k] = n - m (0
        without a neighbour)}; a ``PackedBatch`` gives packed [n_atom, k] arrays.  A neighbour of more than _hip.PAIRING_MAX_ATOMS
        atoms is not comparable: distance inf, ranked last.  Places without a neighbour hold distance inf, id -1, size 0, place -1,
        paired_atom -1.  Raw y.  It refuses what ``match_structures`` refuses, and a shortlist outside k .. 32."""
        k, ms = _hip.check_knn_k(k), _hip.check_match_measure(measure)
        sl = _hip.check_pairing_shortlist(shortlist, k)
        n_at = self._atom_query(inputs, index, "pair_structures", _hip.PAIRING_MAX_ATOMS, batch_size)
        qid = _exclude_ids_arg(inputs, exclude_ids)
        eng = self.engine
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.index_pairing_batch(
            index._ix, rb, k, sl, ms, None if qid is None else qid[s0:s1]),
            {"y": np.zeros(0, np.float32), "score": np.zeros((0, k), np.float32), "id": np.zeros((0, k), np.int64),
             "size": np.zeros((0, k), np.int32), "short_score": np.zeros((0, k), np.float32), "short_place": np.zeros((0, k), np.int32),
             "partner_position": np.zeros((0, k), np.int32), "partner_dist2": np.zeros((0, k), np.float32)})
        _, atoms = eng.index_names(index._ix)  # (host copies: the rows stay on the device)
        pos = cat["partner_position"]
        paired = np.where(pos >= 0, atoms[np.maximum(pos, 0)] if len(atoms) else -1, -1).astype(np.int32)
        surplus = np.where(cat["size"] > 0, np.asarray(n_at, np.int32).reshape(-1, 1) - cat["size"], 0).astype(np.int32)
        out = {"predict_property": cat["y"].reshape(-1, 1), "distance": np.sqrt(cat["score"]),  # (correctly rounded on the host, as nearest)
               "neighbor_id": cat["id"], "neighbor_size": cat["size"], "shortlist_distance": np.sqrt(cat["short_score"]),
               "shortlist_place": cat["short_place"], "paired_atom": paired, "paired_distance": np.sqrt(cat["partner_dist2"]), "surplus": surplus}
        return _repad(out, inputs, "atom", {"paired_atom": -1, "paired_distance": 0})

    def align_structures(self, inputs_a, inputs_b, batch_size=None):
        """The e-th structure of ``inputs_a`` mapped onto the e-th of ``inputs_b`` atom by atom, with no index in sight: two polymorphs,
        a structure before and after relaxation, a substitution series.  ``inputs_b`` is indexed at atom level for the call; the pairs
        (e, e) go through the one-to-one pairing of ``pair_structures`` (scann_index_pairing) on the ``after_Lc`` rows.  Returns
        {"distance": [B] fp32, "atom_map": [B, M_a] int32 -- the atom of b that atom i of a is paired with, -1 where it is surplus or at
        padding --, "atom_distance": [B, M_a] fp32, "surplus": [B] = n_a - n_b, "predict_property": [B, 1] of a and
        "predict_property_b": [B, 1] of b}; ``PackedBatch`` inputs give packed [n_atom] arrays.  A structure of b above
        _hip.PAIRING_MAX_ATOMS atoms is not comparable (distance inf, map -1); one of a, another number of structures or a bad batch_size
        raise ValueError before anything is uploaded.  Raw y."""
        B = count_structures(inputs_a)
        if count_structures(inputs_b) != B:
            raise ValueError("align_structures: %d structures against %d" % (B, count_structures(inputs_b)))
        self._batch_size(batch_size)
        n_a = self._atoms_per_structure(inputs_a, _hip.PAIRING_MAX_ATOMS)
        n_b = self._atoms_per_structure(inputs_b, np.iinfo(np.int32).max)
        if B == 0:
            raise ValueError("align_structures: no structure")
        eng = self.engine
        packed_a = isinstance(inputs_a, _hip.PackedBatch)
        ya, rows = self.predict(inputs_a, outputs=["predict_property", "after_Lc"])
        if not packed_a:
            rows = rows[np.asarray(inputs_a["atom_mask"]).reshape(B, -1) != 0]
        yb = self.predict(inputs_b, outputs=["predict_property"])[0]
        with self._indexed(inputs_b, "atom", batch_size=batch_size) as ix:
            pairs = np.arange(B)
            r = eng.index_pairing(ix._ix, rows, np.concatenate([[0], np.cumsum(n_a)]), pairs, pairs)
            _, atoms = eng.index_names(ix._ix)
        pos = r["partner_position"]
        out = {"distance": np.sqrt(r["score"]), "atom_map": np.where(pos >= 0, atoms[np.maximum(pos, 0)], -1).astype(np.int32),
               "atom_distance": np.sqrt(r["partner_dist2"]), "surplus": (np.asarray(n_a) - np.asarray(n_b)).astype(np.int32),
               "predict_property": ya.reshape(-1, 1), "predict_property_b": yb.reshape(-1, 1)}
        return _repad(out, inputs_a, "atom", {"atom_map": -1, "atom_distance": 0})

    def select_diverse(self, pool, m, reference=None, level="structure", stop_distance=None, batch_size=None):
        """Which ``m`` structures (or atoms, ``level`` "atom") of ``pool`` to label next: greedy k-center selection in the model's latent
        space (``LatentIndex.select``; the core-set rule of Sener & Savarese, ICLR 2018), farthest first from everything in ``reference``
        -- what is labelled already -- and from the picks so far.  Without a reference the call thins ``pool`` to ``m`` representative
        rows.  ``pool`` and ``reference`` are each a ``LatentIndex`` (its level counts, not ``level``) or data as ``build_index`` takes
        it, which is indexed for the call and freed afterwards (ids: 0 .. n-1 in input order).  Returns ``LatentIndex.select``'s dict.
        Bad arguments raise ValueError before anything is uploaded."""
        level_dim(self.config, level)
        m, _ = _hip.check_select_args(m, 0.0)
        stop_dist2_of(stop_distance)
        self._batch_size(batch_size)
        if reference is not None and reference is pool:
            raise ValueError("the reference is the pool itself: every row would be at distance 0")
        for ix in (pool, reference):
            if isinstance(ix, LatentIndex):
                ix.check_model(self)
        if isinstance(pool, LatentIndex):
            level = pool.level
        if isinstance(reference, LatentIndex) and reference.level != level:
            raise ValueError("the reference is a %s-level index, the pool's level is %s" % (reference.level, level))
        with contextlib.ExitStack() as scope:
            pool = scope.enter_context(self._indexed(pool, level, batch_size=batch_size))
            if reference is not None:
                reference = scope.enter_context(self._indexed(reference, level, batch_size=batch_size))
            return pool.select(m, reference=reference, stop_distance=stop_distance)

    def cluster(self, data, k, level="atom", init="kcenter", max_iter=50, stop_changed=0, ids=None, batch_size=None):
        """Which kinds of atom environment (``level`` "atom", the ``after_Lc`` rows) or of structure ("structure", ``bf_property``) the
        model distinguishes: k-means in its latent space, the whole loop on the GPU and bit-reproducible (``LatentIndex.cluster``).
        ``data`` is a ``LatentIndex`` (its level counts, not ``level``) or data as ``build_index`` takes it, which is indexed for the
        call (``ids``: one per structure, default 0 .. n-1) and freed afterwards.  Returns ``(result, clustering)``: ``LatentIndex.cluster``'s
        dict and the ``LatentClustering`` of its centres, which ``assign`` takes and which can be saved.  Bad arguments raise ValueError
        before anything is uploaded."""
        level_dim(self.config, level)
        k, max_iter, stop_changed = _hip.check_kmeans_args(k, max_iter, stop_changed)
        self._batch_size(batch_size)
        if isinstance(init, str):
            if init != "kcenter":
                raise ValueError('init must be "kcenter", %d positions or an array of %d centres, got %r' % (k, k, init))
        elif np.asarray(init).dtype.kind not in "iu":
            _hip.check_kmeans_init(init, level_dim(self.config, _level_of(data, level)))
        with self._indexed(data, level, ids, batch_size) as index:
            result = index.cluster(k, init=init, max_iter=max_iter, stop_changed=stop_changed)
            return result, LatentClustering(result["centre"], index.level, index.dim)

    def silhouette(self, index, labels, sample=None, seed=0, metric="euclidean", route="device", table=False, n_clusters=None):
        """How good a labelling of an index's rows is: the silhouette of every row and its mean, every mean distance over all rows of
        the index from one exact pass over all pairs on the GPU, bit-reproducible (``LatentIndex.silhouette``, whose arguments and dict
        these are).  ``labels`` come from ``cluster``, ``density_peaks`` or ``hierarchy``.  An index of another model and bad
        arguments raise ValueError before any device call."""
        _expect(index, LatentIndex, "index")
        index.check_model(self)
        return index.silhouette(labels, sample=sample, seed=seed, metric=metric, route=route, table=table, n_clusters=n_clusters)

    def choose_k(self, data, ks, level="atom", sample=None, seed=0, metric="euclidean", init="kcenter", max_iter=50, stop_changed=0,
                 route="device", ids=None, batch_size=None):
        """How many kinds of atom environment (``level`` "atom") or of structure ("structure") the model distinguishes: ``cluster`` for
        every k of ``ks``, each scored by the silhouette of its labels, on the GPU and bit-reproducible (``LatentIndex.choose_k``).
        ``data`` is a ``LatentIndex`` (its level counts, not ``level``) or data as ``build_index`` takes it, which is indexed once for
        the call (``ids``: one per structure, default 0 .. n-1) and freed afterwards.  Returns ``(table, clustering)``:
        ``LatentIndex.choose_k``'s dict -- per k the score, the inertia, the Calinski-Harabasz and Davies-Bouldin indices, the sizes,
        ``converged``; "best_k"; the best k's ``cluster`` and ``silhouette`` results -- and the ``LatentClustering`` of the best k's
        centres, which ``assign`` takes and which can be saved.  Bad arguments raise ValueError before anything is uploaded."""
        from .latent_index import choose_k_arg, silhouette_route, silhouette_sample_arg

        level_dim(self.config, _level_of(data, level))
        ks = choose_k_arg(ks)
        silhouette_route(route)
        if metric not in _hip.SILHOUETTE_METRICS:
            raise ValueError("metric must be one of %s, got %r" % (", ".join(_hip.SILHOUETTE_METRICS), metric))
        silhouette_sample_arg(sample if np.ndim(sample) == 0 else None, seed, 0)  # (positions are checked against the index, once it is there)
        _hip.check_kmeans_args(ks[-1], max_iter, stop_changed)
        if isinstance(init, str) and init != "kcenter":
            raise ValueError('init must be "kcenter" for a sweep over k, got %r' % (init,))
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            table = index.choose_k(ks, sample=sample, seed=seed, metric=metric, route=route, init=init, max_iter=max_iter,
                                   stop_changed=stop_changed)
            return table, LatentClustering(table["best"]["centre"], index.level, index.dim)

    def assign(self, inputs, clustering, batch_size=None):
        """The cluster of every structure (or, for an atom-level clustering, every atom) of new ``inputs``, right behind their forward:
        ``nearest`` with k = 1 against an index that holds the centres in order, so bitwise the assignment of the clustering's
        definition (first centre under (distance, index)).  A padded dict gives {"predict_property": [B, 1], "cluster": int32 [B],
        "distance": fp32 [B]} and at atom level [B, M] arrays with -1 / 0 at padded atoms; a ``PackedBatch`` gives packed [n_atom]
        arrays.  Raw y.  A clustering of another width or a bad batch_size raise ValueError before anything is uploaded."""
        _expect(clustering, LatentClustering, "clustering")
        clustering.check_model(self)
        self._batch_size(batch_size)
        r = self.nearest(inputs, clustering.index_on(self), k=1, batch_size=batch_size)
        return {"predict_property": r["predict_property"], "cluster": r["neighbor_id"][..., 0].astype(np.int32), "distance": r["distance"][..., 0]}

    def fit_projection(self, data, m=2, level="structure", ids=None, batch_size=None):
        """The principal-component map of the model's latent space over ``data``: the ``m`` leading axes of the ``bf_property`` rows
        (``level`` "structure") or of the ``after_Lc`` rows ("atom"), mean and covariance computed on the GPU and bit-reproducible
        (``LatentIndex.pca``).  ``data`` is a ``LatentIndex`` (its level counts, not ``level``) or data as ``build_index`` takes it, which
        is indexed for the call (``ids``: one per structure, default 0 .. n-1) and freed afterwards.  Returns ``(result, projection)``:
        ``LatentIndex.pca``'s dict -- the map of ``data`` itself -- and the ``LatentProjection`` that ``project`` takes and that can be
        saved.  Bad arguments raise ValueError before anything is uploaded."""
        dim = level_dim(self.config, _level_of(data, level))
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= dim:
            raise ValueError("m must be an integer in 1 .. %d, got %r" % (dim, m))
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.pca(int(m))

    def fit_embedding(self, data, level="structure", perplexity=10, iterations=(250, 500), exaggeration=12.0, learning_rate="auto",
                      route="device", ids=None, batch_size=None):
        """The neighbour embedding (t-SNE) of the model's latent space over ``data`` in two dimensions (``LatentIndex.embed``): the
        ``bf_property`` rows (``level`` "structure") or the ``after_Lc`` rows ("atom"), the pair repulsion computed exactly on the GPU,
        the map bit-reproducible.  ``data`` is a ``LatentIndex`` (its level counts, not ``level``) or data as ``build_index`` takes it,
        which is indexed for the call (``ids``: one per structure, default 0 .. n-1) and freed afterwards -- ``place`` needs the index,
        so keep one to place new inputs later.  Returns ``(result, embedding)``.  Bad arguments raise ValueError before anything is
        uploaded."""
        level_dim(self.config, _level_of(data, level))
        embed_fit_args(perplexity, iterations, exaggeration, learning_rate, route)
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.embed(perplexity=perplexity, iterations=iterations, exaggeration=exaggeration, learning_rate=learning_rate, route=route)

    def map_quality(self, data_or_index, coords, level="structure", k=15, sample=None, seed=0, route="device", graph=None, ids=None,
                    batch_size=None):
        """Whether a map of the model's latent space can be believed: trustworthiness, continuity and neighbourhood overlap of
        ``coords`` -- an array [N, c], a ``LatentEmbedding`` or the result of ``fit_embedding`` / ``fit_projection`` -- against the
        latent rows themselves, from exact neighbour ranks computed on the GPU, bit-reproducible (``LatentIndex.map_quality``, whose
        arguments and dict these are).  ``data_or_index`` is the ``LatentIndex`` the map was drawn from (its level counts, not
        ``level``) or data as ``build_index`` takes it, which is indexed for the call (``ids``: one per structure, default 0 .. n-1)
        and freed afterwards.  An index of another model and bad arguments raise ValueError before any device call."""
        from .latent_index import silhouette_route, silhouette_sample_arg

        level_dim(self.config, _level_of(data_or_index, level))
        silhouette_route(route)
        silhouette_sample_arg(sample if np.ndim(sample) == 0 else None, seed, 0)  # (positions are checked against the index, once it is there)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 31:
            raise ValueError("k must be an integer in 1 .. 31, got %r" % (k,))
        self._batch_size(batch_size)
        with self._indexed(data_or_index, level, ids, batch_size) as index:
            return index.map_quality(coords, k=k, sample=sample, seed=seed, route=route, graph=graph)

    def choose_perplexity(self, data, perplexities, level="structure", k=15, sample=None, seed=0, iterations=(250, 500), exaggeration=12.0,
                          learning_rate="auto", route="device", ids=None, batch_size=None):
        """Which perplexity draws the most faithful map of the model's latent space over ``data``: ``fit_embedding`` for every
        perplexity of ``perplexities``, each map scored by ``map_quality`` at ``k``, the linear map of ``fit_projection(m=2)`` scored
        beside them (``LatentIndex.choose_perplexity``).  ``data`` is a ``LatentIndex`` (its level counts, not ``level``) or data as
        ``build_index`` takes it, which is indexed once for the call and freed afterwards.  Returns ``(table, embedding)``: per
        perplexity and for "linear" the neighbour overlap, trustworthiness, continuity, LCMC and the R_NX area, "best_perplexity", the
        best map's ``embed`` and ``map_quality`` results -- and its ``LatentEmbedding``.  Bad arguments raise ValueError before
        anything is uploaded."""
        from .latent_index import choose_perplexity_arg, silhouette_sample_arg

        level_dim(self.config, _level_of(data, level))
        perplexities = choose_perplexity_arg(perplexities)
        embed_fit_args(perplexities[0], iterations, exaggeration, learning_rate, route)
        silhouette_sample_arg(sample if np.ndim(sample) == 0 else None, seed, 0)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 31:
            raise ValueError("k must be an integer in 1 .. 31, got %r" % (k,))
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.choose_perplexity(perplexities, k=k, sample=sample, seed=seed, iterations=iterations, exaggeration=exaggeration,
                                           learning_rate=learning_rate, route=route)

    def density_peaks(self, data, level="atom", k=None, bandwidth="auto", neighbours=31, min_density=None, min_delta=None, route="device",
                      ids=None, batch_size=None):
        """Which kinds of atom environment (``level`` "atom", the ``after_Lc`` rows) or of structure ("structure", ``bf_property``) the
        model distinguishes, without a number of clusters and without round clusters: density-peak clustering in its latent space, both
        passes over all pairs exact on the GPU and bit-reproducible (``LatentIndex.density_peaks``).  ``data`` is a ``LatentIndex`` (its
        level counts, not ``level``) or data as ``build_index`` takes it, which is indexed for the call (``ids``: one per structure,
        default 0 .. n-1) and freed afterwards.  Returns ``(result, peaks)``: ``LatentIndex.density_peaks``'s dict and the
        ``LatentPeaks`` whose ``label_of`` labels the positions ``nearest(k=1)`` reports.  Bad arguments raise ValueError before anything
        is uploaded."""
        level_dim(self.config, _level_of(data, level))
        peaks_fit_args(k, bandwidth, neighbours, min_density, min_delta, route)
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.density_peaks(k=k, bandwidth=bandwidth, neighbours=neighbours, min_density=min_density, min_delta=min_delta, route=route)

    def prototypes(self, data, m, level="atom", criticisms=0, bandwidth="auto", neighbours=31, witness="under", assign=True, route="device",
                   ids=None, batch_size=None):
        """The ``m`` atom environments (``level`` "atom", the ``after_Lc`` rows) or structures ("structure", ``bf_property``) that stand
        for all of ``data`` in the model's latent space, and the ``criticisms`` that those do not stand for: MMD-critic, both greedy
        loops exact on the GPU and bit-reproducible (``LatentIndex.prototypes``).  ``data`` is a ``LatentIndex`` (its level counts, not
        ``level``) or data as ``build_index`` takes it, which is indexed for the call (``ids``: one per structure, default 0 .. n-1) and
        freed afterwards.  Returns ``(result, prototypes)``: ``LatentIndex.prototypes``'s dict and the ``LatentPrototypes`` that
        ``nearest_prototype`` takes and that can be saved.  Bad arguments raise ValueError before anything is uploaded."""
        from .latent_index import prototypes_fit_args

        level_dim(self.config, _level_of(data, level))
        prototypes_fit_args(m, criticisms, bandwidth, neighbours, witness, assign, route)
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.prototypes(m, criticisms=criticisms, bandwidth=bandwidth, neighbours=neighbours, witness=witness, assign=assign, route=route)

    def nearest_prototype(self, inputs, prototypes, batch_size=None):
        """The nearest prototype of every structure (or, for atom-level prototypes, every atom) of new ``inputs`` and its distance,
        right behind their forward: a prediction explained by an example.  ``nearest`` with k = 1 against an index that holds the
        prototype rows in order.  A padded dict gives {"predict_property": [B, 1], "prototype": int32 [B] (its place among the
        prototypes), "prototype_id": int64 [B], "distance": fp32 [B]} and at atom level [B, M] arrays plus "prototype_atom", with -1 / 0
        at padded atoms; a ``PackedBatch`` gives packed [n_atom] arrays.  Raw y.  Prototypes of another width or a bad batch_size raise
        ValueError before anything is uploaded."""
        from .latent_index import LatentPrototypes

        _expect(prototypes, LatentPrototypes, "prototypes")
        prototypes.check_model(self)
        self._batch_size(batch_size)
        index = prototypes.index_on(self)
        eng, lvl = self.engine, _hip.KNN_LEVELS[index.level]
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.index_query_batch(index._ix, rb, lvl, 1, None),
                            {"y": np.zeros(0, np.float32), "dist2": np.zeros((0, 1), np.float32), "id": np.zeros((0, 1), np.int64),
                             "atom": np.zeros((0, 1), np.int32), "position": np.zeros((0, 1), np.int32)})
        out = {"predict_property": cat["y"].reshape(-1, 1), "prototype": cat["position"][:, 0], "prototype_id": cat["id"][:, 0],
               "distance": np.sqrt(cat["dist2"][:, 0])}
        if index.level == "atom":
            out["prototype_atom"] = cat["atom"][:, 0]
        return _repad(out, inputs, index.level, {"distance": 0, "prototype": -1, "prototype_id": -1, "prototype_atom": -1})

    def hierarchy(self, data, level="atom", min_samples=5, min_cluster_size=None, route="device", ids=None, batch_size=None):
        """How the kinds of atom environment (``level`` "atom", the ``after_Lc`` rows) or of structure ("structure", ``bf_property``)
        nest, and which rows belong to none: hierarchical clustering in the model's latent space -- single linkage (``min_samples`` 0)
        or HDBSCAN -- on the exact minimum spanning tree, built on the GPU and bit-reproducible (``LatentIndex.hierarchy``).  ``data``
        is a ``LatentIndex`` (its level counts, not ``level``) or data as ``build_index`` takes it, which is indexed for the call
        (``ids``: one per structure, default 0 .. n-1) and freed afterwards.  Returns ``(result, hierarchy)``:
        ``LatentIndex.hierarchy``'s dict -- with ``min_cluster_size`` also the entries of ``hierarchy.clusters(min_cluster_size)`` --
        and the ``LatentHierarchy`` that ``attach`` takes.  Bad arguments raise ValueError before anything is uploaded."""
        level_dim(self.config, _level_of(data, level))
        hierarchy_fit_args(min_samples, route)
        if min_cluster_size is not None:
            check_min_cluster_size(min_cluster_size)
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            result, h = index.hierarchy(min_samples=min_samples, route=route)
        if min_cluster_size is not None:
            result.update(h.clusters(min_cluster_size))
        return result, h

    def attach(self, inputs, hierarchy, index, min_cluster_size, batch_size=None):
        """New ``inputs`` under an existing hierarchy, right behind their forward: every structure (or, at atom level, every atom)
        takes the label its nearest row r of ``index`` -- the ``LatentIndex`` that ``hierarchy`` was built on -- has in
        ``hierarchy.clusters(min_cluster_size)``, from the exact search (scann_index_query_batch, k = 1); -1 if r is noise or if
        max(dist2, core2[r]) >= the squared level at which r's cluster is born (``LatentHierarchy.attach_labels``).  A padded dict
        gives {"predict_property": [B, 1], "global_attention": the scores as ``predict`` returns them, "label": int32 [B],
        "nearest_position": int32 [B], "nearest_id": int64 [B], "nearest_atom": int32 [B], "nearest_distance": fp32 [B]} and at atom
        level [B, M] arrays with -1 / 0 at padded atoms; a ``PackedBatch`` gives packed arrays.  Raw y.  A hierarchy of another width
        or size than the index, or a bad min_cluster_size or batch_size, raise ValueError before anything is uploaded."""
        _expect(hierarchy, LatentHierarchy, "hierarchy")
        _expect(index, LatentIndex, "index")
        hierarchy.check_model(self)
        index.check_model(self)
        if hierarchy.level != index.level or len(hierarchy) != len(index) or len(index) < 1:
            raise ValueError("the hierarchy (%s level, %d rows) was not built on this index (%s level, %d rows)" % (
                hierarchy.level, len(hierarchy), index.level, len(index)))
        clusters = hierarchy.clusters(min_cluster_size)
        self._batch_size(batch_size)
        eng, lvl = self.engine, _hip.KNN_LEVELS[index.level]
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.index_query_batch(index._ix, rb, lvl, 1),
                            {"y": np.zeros(0, np.float32), "ga": np.zeros(0, np.float32), "dist2": np.zeros((0, 1), np.float32),
                             "position": np.zeros((0, 1), np.int32), "id": np.zeros((0, 1), np.int64), "atom": np.zeros((0, 1), np.int32)})
        pos, d2 = cat["position"][:, 0], cat["dist2"][:, 0]
        out = {"predict_property": cat["y"].reshape(-1, 1),
               "global_attention": cat["ga"] if isinstance(inputs, _hip.PackedBatch) else _hip.repad_atoms(cat["ga"], inputs["atom_mask"])[..., None],
               "label": hierarchy.attach_labels(pos, d2, clusters), "nearest_position": pos, "nearest_id": cat["id"][:, 0],
               "nearest_atom": cat["atom"][:, 0], "nearest_distance": np.sqrt(d2)}
        return _repad(out, inputs, index.level, {"label": -1, "nearest_position": -1, "nearest_id": -1, "nearest_atom": -1, "nearest_distance": 0})

    def density(self, inputs, index, bandwidth, batch_size=None):
        """The Gaussian kernel density of every structure (or, for an atom-level index, every atom) of ``inputs`` under the rows of a
        ``LatentIndex``, summed over all its rows on the GPU right behind the forward (scann_index_density_batch): the third
        applicability-domain score beside ``nearest``'s distances and ``project``'s Mahalanobis distance.  ``bandwidth``: the kernel
        width h, a positive number (``density_peaks`` reports the one it used).  A padded dict gives {"predict_property": [B, 1],
        "density": fp64 [B] -- the mean kernel weight to the index's rows, 2^-30 sum / len(index) --, "sum": int64 [B], the exact
        fixed-point sum} and at atom level [B, M] arrays with 0 / -1 at padded atoms; a ``PackedBatch`` gives packed [n_atom] arrays.
        Raw y.  An index of another model or width, a bad bandwidth or batch_size raise ValueError before anything is uploaded."""
        _expect(index, LatentIndex, "index")
        index.check_model(self)
        gamma = _hip.rbf_gamma(bandwidth)
        self._batch_size(batch_size)
        eng, lvl = self.engine, _hip.KNN_LEVELS[index.level]
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.density_batch(index._ix, rb, lvl, gamma),
                            {"y": np.zeros(0, np.float32), "sum": np.zeros(0, np.int64)})
        out = {"predict_property": cat["y"].reshape(-1, 1), "density": density_of_sums(cat["sum"], len(index)), "sum": cat["sum"]}
        return _repad(out, inputs, index.level, {"density": 0, "sum": -1}, dtypes={"density": np.float64})

    def place(self, inputs, embedding, index, batch_size=None):
        """New ``inputs`` on an existing map, right behind their forward: for every structure (or, at atom level, every atom) its 31
        nearest rows of ``index`` -- the ``LatentIndex`` that ``embedding`` maps -- from the exact search (scann_index_query_batch),
        conditional weights calibrated to the embedding's perplexity (``embed_conditional``), coordinates the weighted mean of the
        neighbours' map rows in fp64.  A padded dict gives {"predict_property": [B, 1], "coords": fp32 [B, 2], "nearest_position": int32
        [B], "nearest_id": int64 [B], "nearest_atom": int32 [B], "nearest_distance": fp32 [B]} and at atom level [B, M, 2] / [B, M] arrays
        with 0 / -1 at padded atoms; a ``PackedBatch`` gives packed arrays.  Raw y.  An embedding of another width or index, or a bad
        batch_size, raise ValueError before anything is uploaded."""
        _expect(embedding, LatentEmbedding, "embedding")
        embedding.check_model(self)
        embedding.check_index(index)
        index.check_model(self)
        self._batch_size(batch_size)
        k = min(EMBED_NEIGHBOURS, len(index))
        eng, lvl = self.engine, _hip.KNN_LEVELS[index.level]
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.index_query_batch(index._ix, rb, lvl, k),
                            {"y": np.zeros(0, np.float32), "dist2": np.zeros((0, k), np.float32), "position": np.zeros((0, k), np.int32)})
        out = embedding.place(cat["position"], cat["dist2"])
        out["predict_property"] = cat["y"].reshape(-1, 1)
        return _repad(out, inputs, index.level, {"coords": 0, "nearest_position": -1, "nearest_id": -1, "nearest_atom": -1, "nearest_distance": 0})

    def project(self, inputs, projection, batch_size=None):
        """New ``inputs`` on a ``LatentProjection``'s map, right behind their forward (scann_project_batch): the coordinates, the
        Mahalanobis distance to the distribution the projection was fitted on (an applicability-domain score beside ``nearest``'s
        distances) and the Euclidean distance to its mean.  A padded dict gives {"predict_property": [B, 1], "coordinates": fp32 [B, m],
        "mahalanobis": [B], "distance_to_mean": [B]} and at atom level [B, M, m] / [B, M] arrays with 0 at padded atoms; a
        ``PackedBatch`` gives packed [n_atom, m] / [n_atom] arrays.  Raw y.  A projection of another width or a bad batch_size raise
        ValueError before anything is uploaded."""
        _expect(projection, LatentProjection, "projection")
        projection.check_model(self)
        self._batch_size(batch_size)
        eng, lvl = self.engine, _hip.KNN_LEVELS[projection.level]
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.project_batch(
            rb, lvl, projection.mean, projection.components, projection.scale),
            {"y": np.zeros(0, np.float32), "coords": np.zeros((0, projection.m), np.float32), "md2": np.zeros(0, np.float32), "dist2": np.zeros(0, np.float32)})
        out = projection.finish(cat)
        out["predict_property"] = cat["y"].reshape(-1, 1)
        return _repad(out, inputs, projection.level, {"coordinates": 0, "mahalanobis": 0, "distance_to_mean": 0})

    def fit_head(self, data, targets, level="structure", l2="loo", ids=None, batch_size=None, names=None):
        """A linear readout head for another property on the model's frozen latent space (``LatentIndex.fit_head``): ridge regression of
        ``targets`` on the ``bf_property`` rows (``level`` "structure", one target row per structure) or the ``after_Lc`` rows ("atom",
        one per real atom: a flat array in packed order or one array per structure), the strength chosen by exact leave-one-out on the
        GPU.  ``data`` is a ``LatentIndex`` (its level counts, not ``level``) or data as ``build_index`` takes it, which is indexed for
        the call and freed afterwards.  Returns ``(result, head)``; the ``LatentHead`` is what ``predict_head`` takes and can be saved.
        Bad arguments raise ValueError before anything is uploaded."""
        from .latent_index import head_grid

        lvl = _level_of(data, level)
        level_dim(self.config, lvl)
        t = _hip.check_head_targets(_flat_per_structure(targets, lvl, "targets", np.float32), len(data) if isinstance(data, LatentIndex) else None)
        head_grid(l2)
        if names is not None and len(names) != t.shape[1]:
            raise ValueError("names: %d for %d targets" % (len(names), t.shape[1]))
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.fit_head(t, l2=l2, names=names)

    def predict_head(self, inputs, head, batch_size=None):
        """New ``inputs`` through a ``LatentHead``, right behind their forward (scann_head_batch): the head's prediction of its K
        targets, the predictive standard deviation sqrt(sigma2 (1 + leverage)) of Bayesian linear regression -- an uncertainty beside
        Monte Carlo dropout, ensembles and the latent-space distances -- and the leverage itself.  A padded dict gives {"prediction",
        "std", "leverage": fp32 [B, K], "y": [B, 1] (the model's own raw prediction)} and at atom level [B, M, K] arrays with 0 at padded
        atoms; a ``PackedBatch`` gives packed [n_atom, K] arrays.  A head of another width or a bad batch_size raise ValueError before
        anything is uploaded."""
        _expect(head, LatentHead, "head")
        head.check_model(self)
        self._batch_size(batch_size)
        eng, lvl, K = self.engine, _hip.KNN_LEVELS[head.level], head.k
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.head_batch(
            rb, lvl, head.mean, head.tmean, head.weights, head.components, head.scale, head.lev0),
            {"y": np.zeros(0, np.float32), "pred": np.zeros((0, K), np.float32), "lev": np.zeros((0, K), np.float32)})
        out = head.finish(cat["pred"], cat["lev"])
        out["y"] = cat["y"].reshape(-1, 1)
        return _repad(out, inputs, head.level, {"prediction": 0, "std": 0, "leverage": 0})

    def fit_kernel_head(self, data, targets, level="structure", landmarks=256, bandwidth="loo", l2="loo", ids=None, batch_size=None, names=None):
        """A nonlinear readout head for another property on the model's frozen latent space (``LatentIndex.fit_kernel_head``): ridge
        regression of ``targets`` on Gaussian features to ``landmarks`` of the ``level`` rows, features, moments and leave-one-out all on
        the GPU -- what tells "the representation lacks the information" from "a linear head is too weak".  ``data`` and ``targets`` as
        ``fit_head`` takes them.  Returns ``(result, head)``; the ``LatentKernelHead`` is what ``predict_kernel_head`` takes and can be
        saved.  Bad arguments raise ValueError before anything is uploaded."""
        from .latent_index import head_grid, kernel_bandwidth_arg, kernel_landmarks_arg

        lvl = _level_of(data, level)
        level_dim(self.config, lvl)
        t = _hip.check_head_targets(_flat_per_structure(targets, lvl, "targets", np.float32), len(data) if isinstance(data, LatentIndex) else None)
        head_grid(l2)
        kernel_landmarks_arg(landmarks, len(data) if isinstance(data, LatentIndex) else len(t))
        kernel_bandwidth_arg(bandwidth)
        if names is not None and len(names) != t.shape[1]:
            raise ValueError("names: %d for %d targets" % (len(names), t.shape[1]))
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.fit_kernel_head(t, landmarks=landmarks, bandwidth=bandwidth, l2=l2, names=names)

    def predict_kernel_head(self, inputs, head, batch_size=None):
        """New ``inputs`` through a ``LatentKernelHead``, right behind their forward (scann_rbf_head_batch): the head's prediction of its K
        targets, the predictive standard deviation sqrt(sigma2 (1 + leverage)) of sparse Gaussian process regression -- a nonlinear,
        distance-aware uncertainty --, the leverage, and ``support``, the largest feature of the row: how close it lies to its nearest
        landmark, in [0, 1].  A padded dict gives {"prediction", "std", "leverage": fp32 [B, K], "support": [B], "y": [B, 1] (the
        model's own raw prediction), "ga": [B, M, 1]} and at atom level [B, M, K] / [B, M] arrays with 0 at padded atoms; a
        ``PackedBatch`` gives packed [n_atom, ...] arrays.  A head of another width or a bad batch_size raise ValueError before anything
        is uploaded."""
        _expect(head, LatentKernelHead, "head")
        head.check_model(self)
        self._batch_size(batch_size)
        eng, lvl, h, K = self.engine, _hip.KNN_LEVELS[head.level], head.head, head.k
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.rbf_head_batch(
            rb, lvl, head.landmarks, head.gamma, h.mean, h.tmean, h.weights, h.components, h.scale, h.lev0),
            {"y": np.zeros(0, np.float32), "ga": np.zeros(0, np.float32), "pred": np.zeros((0, K), np.float32),
             "lev": np.zeros((0, K), np.float32), "phi": np.zeros((0, head.m), np.float32)})
        out = head.finish(cat["pred"], cat["lev"], cat["phi"])
        out["y"], out["ga"] = cat["y"].reshape(-1, 1), cat["ga"]
        if not isinstance(inputs, _hip.PackedBatch):
            out["ga"] = _hip.repad_atoms(out["ga"], inputs["atom_mask"], 0)[..., None]
        return _repad(out, inputs, head.level, {"prediction": 0, "std": 0, "leverage": 0, "support": 0})

    def fit_class_head(self, data, labels, level="structure", l2="cv", folds=4, max_iter=100, tol=1e-4, classes=None, ids=None, batch_size=None):
        """A classification head on the model's frozen latent space (``LatentIndex.fit_class_head``): multinomial logistic regression of
        integer ``labels`` (-1: unlabelled) on the ``bf_property`` rows (``level`` "structure", one label per structure) or the
        ``after_Lc`` rows ("atom", one per real atom: a flat array in packed order or one array per structure), the ridge strength
        chosen by cross-validation, every pass over the rows on the GPU.  ``data`` is a ``LatentIndex`` (its level counts, not
        ``level``) or data as ``build_index`` takes it, which is indexed for the call and freed afterwards.  Returns ``(result,
        head)``; the ``LatentClassHead`` is what ``predict_class_head`` takes and can be saved.  Bad arguments raise ValueError
        before anything is uploaded."""
        from .latent_index import class_count_check, class_fit_args, class_labels_arg

        lvl = _level_of(data, level)
        level_dim(self.config, lvl)
        labels = np.asarray(_flat_per_structure(labels, lvl, "labels"))
        lab, cl = class_labels_arg(labels, classes, len(data) if isinstance(data, LatentIndex) else len(labels))
        _, f, _, _ = class_fit_args(l2, folds, max_iter, tol)
        class_count_check(np.bincount(lab[lab >= 0], minlength=len(cl)), cl, f)
        self._batch_size(batch_size)
        with self._indexed(data, level, ids, batch_size) as index:
            return index.fit_class_head(labels, l2=l2, folds=folds, max_iter=max_iter, tol=tol, classes=classes)

    def predict_class_head(self, inputs, head, batch_size=None):
        """New ``inputs`` through a ``LatentClassHead``, right behind their forward (scann_logit_head_batch): the class probabilities,
        the most probable class, its probability, and the entropy of the probabilities in nats (computed on the host) -- an
        uncertainty for a categorical prediction.  A padded dict gives {"probability": fp32 [B, C], "label": int64 [B], "confidence",
        "entropy": fp32 [B], "y": [B, 1] (the model's own raw prediction)} and at atom level [B, M, C] / [B, M] arrays with 0 at
        padded atoms; a ``PackedBatch`` gives packed [n_atom, ...] arrays.  A head of another width or a bad batch_size raise
        ValueError before anything is uploaded."""
        _expect(head, LatentClassHead, "head")
        head.check_model(self)
        self._batch_size(batch_size)
        eng, lvl = self.engine, _hip.KNN_LEVELS[head.level]
        cat = self._run_cat(inputs, batch_size, lambda rb, s0, s1: eng.logit_head_batch(rb, lvl, head.mean, head.weights),
                            {"y": np.zeros(0, np.float32), "prob": np.zeros((0, head.c), np.float32)})
        out = head.finish(cat["prob"])
        out["y"] = cat["y"].reshape(-1, 1)
        return _repad(out, inputs, head.level, {"probability": 0, "label": 0, "confidence": 0, "entropy": 0})

    def predict_uncertainty(self, inputs, samples=30, seed=0, keys=None, rate=None, attention_rate=None, batch_size=None,
                            return_samples=False):
        """Monte Carlo dropout: ``samples`` predictions with the graph's Dropout layers active -- Keras' ``model(x, training=True)`` T
        times -- reduced to their mean and unbiased standard deviation (fp64 sums on the device).  ``rate``: the two Dropout(0.1) layers
        (None: 0.1); ``attention_rate``: the attention-weight Dropout (None: 0.05 with use_drop, else 0).  The masks of a structure depend
        on the structure, ``seed``, the sample number and its key only (``keys``: one integer per structure, default 0), so slicing into
        ``batch_size`` chunks or reordering changes no bit -- and two identical structures with the same key get identical samples.
        Returns {"predict_property": [B, 1], "predict_property_std": [B, 1], "global_attention": [B, M, 1], "global_attention_std":
        [B, M, 1]} (raw y; padded atoms 0; a ``PackedBatch`` without padding gives [n_atom, 1]) and, with ``return_samples``,
        "samples" [T, B, 1].  Bad arguments raise ValueError before anything is uploaded."""
        T = int(samples)
        if T < 2:
            raise ValueError("samples must be >= 2 (the standard deviation divides by samples - 1)")
        p_drop = 0.1 if rate is None else float(rate)
        p_attn = (0.05 if self.config["model"].get("use_drop") else 0.0) if attention_rate is None else float(attention_rate)
        for name, v in (("rate", p_drop), ("attention_rate", p_attn)):
            if not (0.0 <= v < 1.0):
                raise ValueError("%s must lie in [0, 1), got %r" % (name, v))
        packed_in = isinstance(inputs, _hip.PackedBatch)
        B = inputs.n_struct if packed_in else int(np.shape(inputs["neighbors"])[0])
        if keys is not None:
            keys = np.asarray(keys).reshape(-1)
            if keys.shape[0] != B:
                raise ValueError("keys: %d values for %d structures" % (keys.shape[0], B))
            keys = keys.astype(np.uint64)
        eng = self.engine
        # (batch_size 0 has always meant the default here; padded chunks are packed on the host, as in input_gradients)
        parts = self._run_chunks(inputs, batch_size or None, lambda rb, s0, s1: eng.predict_mc(
            rb, T, seed=seed, keys=None if keys is None else keys[s0:s1], p_drop=p_drop, p_attn=p_attn, want_ga=True,
            want_samples=return_samples), host_pack=True)
        out = {"predict_property": np.concatenate([p["y_mean"] for p in parts]).reshape(-1, 1),
               "predict_property_std": np.concatenate([p["y_std"] for p in parts]).reshape(-1, 1)}
        amask = inputs.atom_mask if packed_in else inputs["atom_mask"]  # (a PackedBatch that was never padded has none: [n_atom, 1])
        for name, key in (("global_attention", "ga_mean"), ("global_attention_std", "ga_std")):
            ga = np.concatenate([p[key] for p in parts])
            out[name] = ga.reshape(-1, 1) if amask is None else _hip.repad_atoms(ga, amask)[..., None]
        if return_samples:
            out["samples"] = np.concatenate([p["y_samples"] for p in parts], axis=1)[:, :, None]
        return out

    BIG_PREDICT = 1024   # structures from which `predict(padded arrays)` runs as a pipeline of chunks
    PREDICT_CHUNK = 2048  # structures per chunk: one launch sequence each (16 batches of the reference's 128)
    BIG_SLOTS = 6_000_000  # ... or padded neighbour slots (a launch sequence takes < 8,388,608 atoms / edges: few but large crystals)

    def _select(self, sel):
        """scann_set_outputs for a selection made by _output_selection (None: nothing)"""
        if sel is None:
            self.engine.set_outputs()
        else:
            self.engine.set_outputs(sel[1], after_lc=sel[2], bf_property=sel[3])

    def _pipeline(self, jobs, finish, sel=None, launch=None):
        """The software pipeline behind every batched inference path, on the calling thread.  ``jobs`` yields ``(upload, tag)``;
        ``upload()`` -> ResidentBatch.  Job k + 1 is taken (sliced / packed) and uploaded right after job k's launches are enqueued:
        launches and uploads are asynchronous, so this order alone overlaps host and device.  Up to 2 x streams batches stay in
        flight, batch k on stream k % streams; ``finish(rb, tag)`` collects the OLDEST (download, outputs), in job order, and the
        batch is then released without a device-wide synchronisation, so the device keeps running the younger ones.  ``sel``: the
        output selection, set before the first launch and cleared on every exit.  ``launch(rb, slot)``: what is enqueued per batch
        (None: the handle's forward).  On any error every batch uploaded and not yet released is freed, once, and the error propagates.  (A producer thread for slicing + upload, rounds 3-4, cost more in
        Python thread hand-offs than it hid: bench.py end_to_end 1.70-1.72 M -> 1.81 M molecules/s without it.)"""
        eng = self.engine
        ns = eng.num_streams()
        launch = launch or eng.forward_resident
        pending = []  # (batch, tag) in flight, oldest first
        rb = None  # uploaded, not yet in flight

        def fetch_oldest():
            finish(*pending[0])
            pending.pop(0)[0].release()

        try:
            if sel is not None:
                self._select(sel)
            for k, (upload, tag) in enumerate(jobs):
                rb = upload()
                if len(pending) >= 2 * ns:
                    fetch_oldest()
                launch(rb, k % ns)
                pending.append((rb, tag))
                rb = None
            while pending:
                fetch_oldest()
        finally:
            if rb is not None:
                rb.free()
            for b, _ in pending:
                b.free()
            if sel is not None:
                self._select(None)

    def _batch_size(self, batch_size):
        """The structures per chunk of a batched call -- None: hyper.batch_size; anything below 1 is a ValueError"""
        bs = int(self.config["hyper"]["batch_size"] if batch_size is None else batch_size)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        return bs

    def _run_chunks(self, data, batch_size, call, host_pack=False):
        """A synchronous per-batch engine call over ``data`` (what ``batch_jobs`` takes), ``batch_size`` structures at a time:
        ``call(rb, s0, s1)`` for the resident batch of structures s0 .. s1 - 1, its results as a list in chunk order.  The calls run
        their own forward, so nothing is enqueued ahead: the pipeline uploads chunk k + 1 before chunk k is computed and frees every
        batch once, also on an error.  A bad batch_size raises ValueError before anything is uploaded.  ``host_pack``: padded chunks go
        through the host packer whatever the model would choose."""
        eng, parts, at = self.engine, [], [0]

        def finish(rb, cnt):
            parts.append(call(rb, at[0], at[0] + cnt))
            at[0] += cnt

        upload = (lambda chunk: eng.upload(_hip.pack_inputs(chunk))) if host_pack else None
        self._pipeline(batch_jobs(self, data, self._batch_size(batch_size), upload), finish, launch=lambda rb, slot: None)
        return parts

    def _run_cat(self, inputs, batch_size, call, empty):
        """``_run_chunks`` for a call that returns a dict of arrays per chunk: the entries ``empty`` names, concatenated in chunk order;
        ``empty`` itself -- the prototype, {name: array of no rows} -- for inputs without a structure."""
        parts = self._run_chunks(inputs, batch_size, call)
        return {n: np.concatenate([p[n] for p in parts]) if parts else empty[n] for n in empty}

    @contextlib.contextmanager
    def _indexed(self, data, level, ids=None, batch_size=None):
        """The ``LatentIndex`` an analysis runs on: ``data`` itself if it is one of this model (ValueError otherwise), else ``data``
        indexed at ``level`` for the length of the ``with`` block and freed on the way out, also on an error."""
        if isinstance(data, LatentIndex):
            data.check_model(self)
            yield data
            return
        index = self.build_index(data, level=level, ids=ids, batch_size=batch_size)
        try:
            yield index
        finally:
            index.free()

    def _upload_padded(self, inputs):
        """A padded input dict (or row views of one) -> resident batch: feature = "atomic" without ring on an inference handle is
        packed to CSR on the DEVICE (the host reads its masks only, as forward_padded does), anything else by the native host packer."""
        m, eng = self.config["model"], self.engine
        if m["feature"] == "atomic" and not m["use_ring"] and not eng.training:
            return eng.upload_padded(inputs)
        return eng.upload(_hip.pack_inputs(inputs))

    def _read_outputs(self, rb, sel):
        """the packed outputs of a downloaded batch: {name: array} for the names beyond y and the GlobalAttention scores"""
        eng, out = self.engine, {}
        for k in sel[1]:
            out["local_attention_%d" % k] = eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, k)
        if sel[2]:
            out["after_Lc"] = eng.read_output(rb, _hip.OUT_AFTER_LC)
        if sel[3]:
            out["bf_property"] = eng.read_output(rb, _hip.OUT_BF_PROPERTY)
        return out

    def _assemble(self, sel, y, ga_pad, packed, atom_mask=None, neighbor_mask=None):
        """the list predict(outputs=...) returns; atom_mask / neighbor_mask None: per-edge / per-atom outputs stay packed"""
        res = []
        for n in sel[0]:
            if n == "predict_property":
                res.append(y.reshape(-1, 1))
            elif n == "global_attention":
                res.append(ga_pad)
            elif n.startswith("local_attention_"):
                a = packed["local_attention_%d" % int(n[16:])]
                res.append(a if atom_mask is None else _hip.repad_local_attention(a, atom_mask, neighbor_mask))
            elif n == "after_Lc":
                res.append(packed[n] if atom_mask is None else _hip.repad_atoms(packed[n], atom_mask))
            else:
                res.append(packed[n])
        return res

    def _predict_outputs(self, inputs, sel):
        """one batch through the resident pipeline with the selected outputs on (the handle's selection is cleared afterwards)"""
        eng, got = self.engine, []
        is_packed = isinstance(inputs, _hip.PackedBatch)

        def finish(rb, _):
            y, ga = eng.download(rb, want_ga=True)
            got.extend((y, rb.packed.repad_ga(ga), self._read_outputs(rb, sel)))

        upload = functools.partial(eng.upload if is_packed else self._upload_padded, inputs)
        self._pipeline([(upload, None)], finish, sel)
        if is_packed:
            return self._assemble(sel, *got)
        return self._assemble(sel, *got, inputs["atom_mask"], inputs["neighbor_mask"])

    def _predict_chunked(self, inputs, sel=None):
        """`model.predict(x)` on a WHOLE padded dataset (what the reference's evaluate / predict scripts do with Keras, which batches
        internally: scann_model.py:266,316): rows are cut into chunks -- views, nothing is copied -- and software-pipelined on this
        thread: chunk k + 1 is packed and uploaded (host, native code) while the device runs chunk k (launches are asynchronous),
        a rolling window of chunks stays in flight over the handle's streams, results are fetched oldest first.  One launch sequence
        for everything would leave the device idle while the host packs 45 M neighbour slots, and the host idle afterwards."""
        eng = self.engine
        B = len(inputs["atom_mask"])
        nb = np.shape(inputs["neighbors"])
        want_ga = self.infer if sel is None else "global_attention" in sel[0]
        outs = []  # per chunk: {name: packed array}
        # at least four chunks (the first chunk's packing is the only host work the device waits for), at most PREDICT_CHUNK
        # structures and BIG_SLOTS * 2 / 3 padded slots each
        C = min(self.PREDICT_CHUNK, max(512, -(-B // 4 // 128) * 128))
        C = max(1, min(C, (self.BIG_SLOTS * 2 // 3) // max(1, int(nb[1]) * max(1, int(nb[2])))))
        ys, gas = [], []

        def finish(rb, first):
            try:
                y, ga = eng.download(rb, want_ga=want_ga)
                if sel is not None:
                    outs.append(self._read_outputs(rb, sel))
            except _hip.ScannHipError as e:
                # (a device-packed chunk reports bad input only here, up to a window of chunks after it was uploaded: say WHICH chunk)
                raise _hip.ScannHipError(e.code, "%s [structures %d..%d of this call]" % (e.detail, first, min(first + C, B) - 1)) from e
            ys.append(y)
            if want_ga:
                gas.append(ga)

        # one job per chunk of rows (views), tagged with its first structure
        self._pipeline(((functools.partial(self._upload_padded, {key: v[i:i + C] for key, v in inputs.items()}), i)
                        for i in range(0, B, C)), finish, sel)
        y = np.concatenate(ys).reshape(-1, 1)
        if not want_ga and sel is None:
            return y
        amask = np.asarray(inputs["atom_mask"]).reshape(B, -1) != 0
        ga_pad = None
        if want_ga:
            ga_pad = _hip.repad_atoms(np.concatenate(gas), amask)[..., None]  # softmax of -1e9 -> 0 on padded atoms
        if sel is None:
            return [y, ga_pad]
        # chunks are consecutive structures: their packed outputs, concatenated, are the whole batch's packed outputs
        packed = {n: np.concatenate([o[n] for o in outs]) for n in (outs[0] if outs else {})}
        return self._assemble(sel, y, ga_pad, packed, amask, inputs["neighbor_mask"])

    @staticmethod
    def default_group(dataset):
        """Batches fused per launch sequence when the caller does not say: about 1,024 structures (8 batches of 128) -- two such groups
        in flight on the handle's two streams measured best (tools/e2e_size.py: 1.78 M molecules/s; 1.64 M at 4, 1.69 M at 12)."""
        bs = int(getattr(dataset, "batch_size", 0) or 0)
        return max(1, 1024 // bs) if bs > 0 else 8

    def predict_dataset(self, dataset, group=None, want_ga=False, outputs=None):
        """Pipelined inference over a whole ``PackedDataset`` (or any sequence of ``(PackedBatch | inputs dict, target)``):
        batches are fused ``group`` at a time into one launch sequence, spread over the handle's streams, and fetched at
        the end -- the throughput path behind ``SCANN.evaluate`` / ``predict_model.py``.  Returns ``(y [N], ga list | None,
        targets [N])`` in dataset order.

        ``outputs`` (names ``local_attention_<k>``, ``after_Lc``, ``bf_property``): a fourth element, ``{name: [one array per
        structure]}`` in dataset order, each as ``predict(batch, outputs=...)`` returns it for that structure's own batch of the
        dataset (fused groups are split back into batches): [num_head, M, N] / [M, global_dim] / [dense_out], M and N the
        batch's largest structure and neighbour count.

        One group is one job of ``_pipeline``: group k + 1 is sliced and uploaded on the calling thread right after group k's
        launches are enqueued, a rolling window of 2 x streams groups stays in flight, results are fetched oldest first."""
        eng = self.engine
        ys, gas, ts = [], [], []
        group = int(group) if group else self.default_group(dataset)
        sel = None
        if outputs is not None:
            sel = _output_selection(outputs, int(self.config["model"]["n_attention"]))
            if "predict_property" in sel[0] or "global_attention" in sel[0]:
                raise ValueError("predict_dataset returns predict_property and global_attention as y and ga (want_ga=True)")
        per_struct = {n: [] for n in sel[0]} if sel is not None else None
        n = len(dataset)
        grouped = getattr(dataset, "batches", None)  # PackedDataset: a whole group with one native slice call

        def jobs():  # tag: (targets, the group's PackedBatch, structures per dataset batch)
            for g0 in range(0, n, group):
                if grouped is not None:
                    pk, tgt = grouped(g0, min(n, g0 + group))
                    tg, counts = [np.asarray(tgt, dtype=np.float32)], None
                    if sel is not None:  # (a dataset batch holds batch_size structures, the last one the rest)
                        bs = int(dataset.batch_size)
                        counts = [min(bs, pk.n_struct - j) for j in range(0, pk.n_struct, bs)]
                else:
                    parts, tg = [], []
                    for i in range(g0, min(n, g0 + group)):
                        item, tgt = dataset[i]
                        parts.append(item if isinstance(item, _hip.PackedBatch) else _hip.pack_inputs(item))
                        tg.append(np.asarray(tgt, dtype=np.float32))
                    pk = _hip.concat_packed(parts) if len(parts) > 1 else parts[0]
                    counts = [p.n_struct for p in parts]
                yield functools.partial(eng.upload, pk), (tg, pk, counts)

        def finish(rb, tag):
            tg, pk, counts = tag
            y, ga = eng.download(rb, want_ga=want_ga)
            if sel is not None:
                self._split_outputs(self._read_outputs(rb, sel), pk, counts, per_struct)
            ys.append(y)
            if want_ga:
                gas.append(ga)
            ts.extend(tg)

        self._pipeline(jobs(), finish, sel)
        if not ys:
            res = np.zeros(0, np.float32), (np.zeros(0, np.float32) if want_ga else None), np.zeros(0, np.float32)
        else:
            res = np.concatenate(ys), (np.concatenate(gas) if want_ga else None), np.concatenate(ts)
        return res if sel is None else res + (per_struct,)

    def _split_outputs(self, packed, pk, counts, per_struct):
        """Packed outputs of one fused group (PackedBatch ``pk``, ``counts`` structures per dataset batch) -> one array per structure,
        appended to ``per_struct``: what the padded predict of that structure's own batch returns for it (each dataset batch is
        repadded as a whole; its structures are views of that array)."""
        mol = np.asarray(pk.mol_offset, dtype=np.int64)
        eoff = np.asarray(pk.edge_offset, dtype=np.int64)
        deg = np.diff(eoff)
        s0 = 0
        for cnt in counts:
            a0, a1 = int(mol[s0]), int(mol[s0 + cnt])
            sizes = np.diff(mol[s0:s0 + cnt + 1])
            M = int(sizes.max()) if cnt else 0
            N = int(deg[a0:a1].max()) if a1 > a0 else 0
            st = np.repeat(np.arange(cnt), sizes)  # structure of each atom of the batch, and its slot in the structure
            slot = np.arange(a1 - a0) - np.repeat(mol[s0:s0 + cnt] - a0, sizes)
            amask = np.zeros((cnt, M), dtype=bool)
            amask[st, slot] = True
            em = np.zeros((cnt, M, N), dtype=bool)  # the batch's neighbour mask
            em[st, slot] = np.arange(N)[None, :] < deg[a0:a1, None]
            for name, arr in packed.items():
                if name.startswith("local_attention_"):
                    v = _hip.repad_local_attention(arr[eoff[a0]:eoff[a1]], amask, em)
                elif name == "after_Lc":
                    v = _hip.repad_atoms(arr[a0:a1], amask)
                else:
                    v = arr[s0:s0 + cnt]
                per_struct[name].extend(list(v))
            s0 += cnt

    def summary(self):
        print("SCANN HIP model: %d parameters, %d local-attention layers, g_update=%s" % (
            self.count_params(), self.config["model"]["n_attention"], self.config["model"]["g_update"]))


def _read_container(path, config=None):
    with open(path, "rb") as f:
        magic = f.read(8)
    if magic.startswith(b"\x89HDF"):  # a Keras full-model HDF5 checkpoint of the reference (scann_model.py:166-177)
        from .keras_import import load_keras_h5

        return load_keras_h5(path, config)
    z = np.load(path, allow_pickle=False)
    cfg = json.loads(str(z["__config__"]))
    return cfg, {k: z[k] for k in z.files if k != "__config__"}


def load_model(path, custom_objects=None, infer=False, config=None, outputs=None):
    """``tf.keras.models.load_model`` counterpart (scann_model.py:79,87,323): this package's weight container, or a Keras
    HDF5 checkpoint written by the reference (imported by ``keras_import``; pass the run's ``config`` for the keys the file
    does not determine)."""
    cfg, weights = _read_container(path, config)
    if config is not None:  # the caller's yaml wins for everything but the architecture (hyper.target selects the mrelu head)
        cfg["hyper"].update({k: v for k, v in config.get("hyper", {}).items() if k != "target" or "target" not in cfg["hyper"]})
    return HipModel(cfg, weights, infer=infer, outputs=outputs)


def create_model_pretrained(pretrained):
    model = load_model(pretrained)
    model.summary()
    return model


def create_model(config, seed=None):
    """The graph builder (scann_model.py:329-453): returns a model with fresh Keras-default weights."""
    model = HipModel(config, seed=seed)
    model.summary()
    return model


class SCANN:
    """API facade, same constructor and methods as the reference class (scann_model.py:42-319)."""

    def __init__(self, config=None, pretrained="", mode="train"):
        self.config = normalize_config(config)
        self.model = None
        self.mean, self.std = 0, 1
        if "target_mean" in self.config["hyper"]:
            self.mean = float(self.config["hyper"]["target_mean"])
            self.std = float(self.config["hyper"]["target_std"])
        if mode == "train" or mode == "eval":
            if pretrained:
                print("load pretrained model from ", pretrained, "\n")
                self.model = create_model_pretrained(pretrained)
                self.config["hyper"]["pretrained"] = pretrained
                if mode == "train" and self.config["hyper"]["reset"]:
                    # the head for a new target: the matched tensors from the model's own initialisers (under --deterministic the
                    # draw comes from hyper.seed, like a fresh model's)
                    from .finetune import reset_weights

                    seed = int(self.config["hyper"].get("seed", 0)) if self.config["hyper"]["deterministic"] else None
                    w, done = reset_weights(self.model.get_weights(), self.model.engine.weight_specs(), self.config["hyper"]["reset"], seed)
                    self.model.set_weights(w)
                    print("re-initialised %d tensors: %s\n" % (len(done), ", ".join(done)))
            elif self.config["hyper"]["deterministic"]:
                # reproducible run: the initial weights come from hyper.seed as well, not from fresh OS entropy
                self.model = create_model(self.config, seed=int(self.config["hyper"].get("seed", 0)))
            else:
                self.model = create_model(self.config)
        elif mode == "data":  # the configuration and its dataset only (prepare_dataset), no model: predict_model.py --with
            pass
        else:
            self.model = load_model(pretrained, infer=True, config=self.config)

    @classmethod
    def load_model_infer(cls, path, outputs=None):
        """scann_model.py:86-91 builds a Keras sub-model that returns [prediction, GlobalAttention scores]; ``outputs`` (layer
        names: predict_property, global_attention, local_attention_<k>, after_Lc, bf_property) builds the sub-model that returns
        those, in that order."""
        return load_model(path, infer=True, outputs=outputs)

    @classmethod
    def load_model(cls, path):
        return create_model_pretrained(path)

    def prepare_dataset(self, split=True, packed=False):
        """Reference behaviour (scann_model.py:98-161).  ``packed=True`` (extension) builds ``PackedDataset`` iterators:
        the object arrays are converted once to flat CSR and batches become slices; they yield
        ``(PackedBatch, target)`` instead of ``(inputs dict, target)``."""
        from ..utils.datagenerator import DataIterator
        from ..utils.general import load_dataset, split_data
        from ..utils.packed_dataset import PackedDataset

        if packed:
            DataIterator = PackedDataset  # noqa: F811  (same constructor signature)

        hy, mo = self.config["hyper"], self.config["model"]
        data_energy, data_neighbor = load_dataset(
            use_ref=hy["use_ref"], use_ring=mo["use_ring"], dataset=hy["data_energy_path"],
            dataset_neighbor=hy["data_nei_path"], target_prop=hy["target"])
        if hy["scaler"]:
            target = [d[1] for d in data_energy]
            self.mean, self.std = np.mean(target, dtype="float32"), np.std(target, dtype="float32")
            print("Normalize dataset property with mean: ", self.mean, " , std: ", self.std, "\n")
            data_energy[:, 1] = (data_energy[:, 1] - self.mean) / self.std
        hy["target_mean"] = str(self.mean)
        hy["target_std"] = str(self.std)
        hy["data_size"] = len(data_energy)
        kw = dict(batch_size=hy["batch_size"], use_ring=mo["use_ring"], feature=mo["feature"], g_update=mo["g_update"],
                  atomic_features=hy.get("cgcnn_table"))  # cgcnn: path of the element table (else SCANN_CGCNN_TABLE)
        if split:
            train, valid, test, extra = split_data(len_data=len(data_energy), test_percent=hy["test_percent"],
                                                   train_size=hy["train_size"], test_size=hy["test_size"])
            assert len(extra) == 0, "Split was inexact {} {} {} {}".format(len(train), len(valid), len(test), len(extra))
            print("Number of train data : ", len(train), " , Number of valid data: ", len(valid),
                  " , Number of test data: ", len(test), "\n")
            self.trainIter, self.validIter, self.testIter = [
                DataIterator(data_neighbor=data_neighbor[idx], data_energy=data_energy[idx],
                             shuffle=(len(idx) == len(train)), **kw)
                for idx in (train, valid, test)]
            return train, valid, test
        self.dataIter = DataIterator(data_neighbor=data_neighbor, data_energy=data_energy, **kw)

    def _out_dir(self):
        return "{}_{}".format(self.config["hyper"]["save_path"], self.config["hyper"]["target"])

    def train(self, epochs=1000):
        """``compile`` + ``fit`` of the reference (scann_model.py:199-245): RMSE loss + l2 regularisers, Adam with the
        legacy decay, CosineDecay or SGDR schedule, best-val_mae checkpoint, early stopping; afterwards the model is
        dropped so that ``evaluate`` reloads the best checkpoint, exactly like the reference."""
        import yaml

        from .trainer import fit

        os.makedirs("{}/models/".format(self._out_dir()), exist_ok=True)
        if int(os.environ.get("RANK", "0")) == 0:
            yaml.safe_dump(self.config, open("{}/config.yaml".format(self._out_dir()), "w"), default_flow_style=False)

        class _Hist:
            pass

        self.hist = _Hist()
        self.hist.history = fit(self, epochs)
        del self.model

    def evaluate(self, gpus=None):
        """Test-set loop of the reference (scann_model.py:247-313): predict every batch, report
        R2 and MAE * std, write report.txt.  ``gpus`` (or ``hyper.gpus``) > 1 spreads the batches over that many
        devices of the node from this process (scann.parallel.MultiGpuPredictor; no collective)."""
        from sklearn.metrics import mean_absolute_error, r2_score

        if int(os.environ.get("WORLD_SIZE", "1")) > 1 and int(os.environ.get("RANK", "0")) != 0:
            # data-parallel job: the test set, report.txt and hist_data.npy belong to rank 0 alone (the ranks hold the same
            # model after training; trainer.fit ends with a barrier, so the best checkpoint is complete before rank 0 loads it)
            return None, None
        if not hasattr(self, "model") or self.model is None:
            print("Load best validation weight for predicting testset", "\n")
            t = self.config["hyper"]["target"]
            self.model = load_model("{}/models/model_{}.h5".format(self._out_dir(), t))
        data = self.dataIter if hasattr(self, "dataIter") else self.testIter
        runner = self.model
        n_gpu = int(gpus if gpus is not None else self.config["hyper"].get("gpus", 1))
        if n_gpu > 1:
            from ..parallel import MultiGpuPredictor, MultiProcessPredictor

            # hyper.gpu_processes: one worker PROCESS per device instead of one thread (no shared interpreter; PackedDataset only)
            if self.config["hyper"].get("gpu_processes") and hasattr(data, "batches"):
                runner = MultiProcessPredictor(self.config, self.model.get_weights(), devices=list(range(n_gpu)))
            else:
                runner = MultiGpuPredictor(self.config, self.model.get_weights(), devices=list(range(n_gpu)))
        yp, _, yt = runner.predict_dataset(data)  # same per-batch results as the reference's predict loop (:264-271)
        if hasattr(runner, "close"):
            runner.close()
        y_predict, y = list(yp), list(yt)
        mae = mean_absolute_error(y, y_predict) * self.std
        r2 = r2_score(y, y_predict)
        print("Result for testset ", self.config["hyper"]["target"], " : R2 score: ", r2, " and MAE: ", mae)
        os.makedirs(self._out_dir(), exist_ok=True)
        with open("{}/report.txt".format(self._out_dir()), "w") as f:
            if hasattr(self, "hist"):  # scann_model.py:292-311
                f.write("Training MAE: " + str(min(self.hist.history["mae"]) * self.std) + "\n")
                f.write("Val MAE: " + str(min(self.hist.history["val_mae"]) * self.std) + "\n")
            f.write("Test MAE: " + str(mae) + ", Test R2: " + str(r2))
        if hasattr(self, "hist"):
            np.save("{}/hist_data.npy".format(self._out_dir()), np.array([y_predict, y, self.hist.history], dtype=object))
            print("Saved model record for dataset")
        return mae, r2

    def input_gradients(self, ip, wrt=("neighbor_distance", "neighbor_weight"), batch_size=None):
        """HipModel.input_gradients in the units of the target: gradients scaled by the target's std and the prediction
        de-normalised, as predict_data does."""
        out = self.model.input_gradients(ip, wrt=wrt, batch_size=batch_size)
        y = out.pop("predict_property")
        res = {k: v * self.std for k, v in out.items()}
        res["predict_property"] = y * self.std + self.mean
        return res

    def pair_structures(self, ip, index, k=5, shortlist=32, measure="chamfer", exclude_ids=None, batch_size=None):
        """HipModel.pair_structures with ``predict_property`` in the units of the target (times std plus mean, as predict_data); the
        distances, the atom maps and the counts live in latent space and pass through as they are."""
        out = self.model.pair_structures(ip, index, k=k, shortlist=shortlist, measure=measure, exclude_ids=exclude_ids, batch_size=batch_size)
        out["predict_property"] = out["predict_property"] * self.std + self.mean
        return out

    def align_structures(self, ip_a, ip_b, batch_size=None):
        """HipModel.align_structures with both predictions, ``predict_property`` and ``predict_property_b``, in the units of the target."""
        out = self.model.align_structures(ip_a, ip_b, batch_size=batch_size)
        for k in ("predict_property", "predict_property_b"):
            out[k] = out[k] * self.std + self.mean
        return out

    def atom_contributions(self, ip, mode="leave_one_out", batch_size=None):
        """HipModel.atom_contributions in the units of the target: ``y`` and ``ablated`` de-normalised as predict_data does (times std
        plus mean, real atoms only), ``contribution`` -- a difference of two predictions -- times std only."""
        out = self.model.atom_contributions(ip, mode=mode, batch_size=batch_size)
        real = (np.asarray(ip["atom_mask"]).reshape(out["order"].shape) != 0)[..., None]
        out["y"] = out["y"] * self.std + self.mean
        out["ablated"] = np.where(real, out["ablated"] * self.std + self.mean, 0).astype(np.float32)
        if "contribution" in out:
            out["contribution"] = out["contribution"] * self.std
        return out

    def atom_shapley(self, ip, permutations=64, seed=0, keys=None, batch_size=None):
        """HipModel.atom_shapley in the units of the target: ``shapley`` and ``stderr`` -- differences of predictions -- times std, ``y``,
        ``baseline`` and ``full`` times std plus mean, as predict_data does."""
        out = self.model.atom_shapley(ip, permutations=permutations, seed=seed, keys=keys, batch_size=batch_size)
        for k in ("shapley", "stderr"):
            out[k] = out[k] * self.std
        for k in ("y", "baseline", "full"):
            out[k] = out[k] * self.std + self.mean
        return out

    def predict_uncertainty(self, ip, samples=30, seed=0, keys=None, rate=None, attention_rate=None, batch_size=None, return_samples=False):
        """HipModel.predict_uncertainty in the units of the target, as predict_data de-normalises: the mean times std plus mean, the
        standard deviation and the samples times |std|; the GlobalAttention scores as they are."""
        out = self.model.predict_uncertainty(ip, samples=samples, seed=seed, keys=keys, rate=rate, attention_rate=attention_rate,
                                             batch_size=batch_size, return_samples=return_samples)
        out["predict_property"] = out["predict_property"] * self.std + self.mean
        out["predict_property_std"] = out["predict_property_std"] * abs(self.std)
        if "samples" in out:
            out["samples"] = out["samples"] * self.std + self.mean
        return out

    @classmethod
    def load_ensemble(cls, model_dirs, device=None):
        """Several trained models of one architecture -- K targets of one dataset, or K seeds of one target -- as one model set
        (``scann.models.ModelSet``): ``model_dirs`` are training output folders (``config.yaml`` + ``models/model_<target>.h5``).
        Returns an ``Ensemble`` whose ``predict(inputs)`` de-normalises each member with its own target mean / std."""
        from .model_set import Ensemble

        return Ensemble(model_dirs, device=device)

    def predict_data(self, ip):
        out = self.model.predict(ip)
        if isinstance(out, list):  # infer mode (the reference tests len(out) == 2, scann_model.py:317)
            return out[0] * self.std + self.mean, out[1]
        return out * self.std + self.mean


# The rest of the facade: HipModel's analysis methods under the same names.  (name, the one entry of the result that is a prediction of
# the model's own target and is de-normalised as predict_data does -- None: the result passes through as it is; everything else lives in
# latent space, on a map or in the units of a head's own targets).  Signature and defaults are HipModel's: they exist once.
FACADE = (("attention_rollout", "predict_property"), ("build_index", None), ("nearest", "predict_property"),
          ("match_structures", "predict_property"), ("select_diverse", None), ("cluster", None), ("silhouette", None), ("choose_k", None),
          ("assign", "predict_property"), ("fit_projection", None), ("fit_embedding", None), ("map_quality", None), ("choose_perplexity", None),
          ("density_peaks", None), ("hierarchy", None), ("attach", "predict_property"), ("density", "predict_property"),
          ("place", "predict_property"), ("project", "predict_property"), ("fit_head", None), ("predict_head", "y"), ("fit_kernel_head", None),
          ("predict_kernel_head", "y"), ("fit_class_head", None), ("predict_class_head", "y"))


def _facade(name, key):
    inner = getattr(HipModel, name)

    @functools.wraps(inner)
    def method(self, *args, **kwargs):
        out = getattr(self.model, name)(*args, **kwargs)
        if key is not None:
            out[key] = out[key] * self.std + self.mean
        return out

    method.__qualname__ = "SCANN." + name
    method.__doc__ = ("HipModel.%s as it is.\n\n" % name if key is None else
                      "HipModel.%s with ``%s`` in the units of the target (times std plus mean, as predict_data).\n\n" % (name, key)) + inner.__doc__
    return method


# the radius search, by the same rule (a table of its own: tests/test_python_layer_host.py counts the entries of the one above)
FACADE_RADIUS = (("within", "predict_property"), ("duplicates", None))
# ... and the prototypes
FACADE_PROTO = (("prototypes", None), ("nearest_prototype", "predict_property"))

for _name, _key in FACADE + FACADE_RADIUS + FACADE_PROTO:
    setattr(SCANN, _name, _facade(_name, _key))

"""Host tests of the input gradients (HipModel.input_gradients, scann_input_grads): the fp64 restatement in tests/input_grad_ref.py
against central directional finite differences of tests/torch_ref.forward_packed, the Python layer (name checks, re-padding, slicing)
against a stand-in engine, and the new kernels' descriptors in the built library.  No GPU."""
import types

import numpy as np
import pytest

import abi_checks
import scann_oracle as so

pytest.importorskip("torch")


def make_batch(n=4, seed=1, L=2, target=None, **over):
    from scann import _hip

    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if target:
        cfg["hyper"]["target"] = target
    ring, cg = bool(cfg["model"]["use_ring"]), cfg["model"]["feature"] == "cgcnn"
    w = so.init_weights(cfg, 3, perturb=True)
    de, dn = so.synth_dataset(n, seed, use_ring=ring)
    inputs, _ = so.pad_batch(de, dn, cfg["model"]["g_update"], use_ring=ring)
    if cg:
        inputs["atomic"] = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")[inputs["atomic"]]
    return cfg, w, inputs, _hip.pack_inputs(inputs)


def _as64(pk, **repl):
    """the attributes forward_packed reads, in float64 (a PackedBatch holds float32: a finite-difference step would round away)"""
    ns = types.SimpleNamespace(atomic=pk.atomic, mol_offset=pk.mol_offset, edge_offset=pk.edge_offset, edge_col=pk.edge_col,
                               edge_dist=pk.edge_dist.astype(np.float64), edge_weight=pk.edge_weight.astype(np.float64),
                               ring=None if pk.ring is None else pk.ring.astype(np.float64),
                               cgcnn=None if pk.cgcnn is None else pk.cgcnn.astype(np.float64),
                               n_atom=pk.n_atom, n_edge=pk.n_edge, n_struct=pk.n_struct)
    for k, v in repl.items():
        setattr(ns, k, v)
    return ns


FIELD = {"neighbor_distance": "edge_dist", "neighbor_weight": "edge_weight", "ring_aromatic": "ring", "atomic": "cgcnn"}

FD_CASES = {
    "g_update": {},
    "base": dict(g_update=False),
    "no_attn_norm": dict(use_attn_norm=False),
    "no_ga_norm": dict(use_ga_norm=False),
    "base_no_norms": dict(g_update=False, use_attn_norm=False, use_ga_norm=False),
    "ring": dict(use_ring=True),
    "cgcnn_base": dict(feature="cgcnn", g_update=False),
}


@pytest.mark.parametrize("case", list(FD_CASES))
def test_reference_matches_directional_finite_differences(case):
    """d y_s / d x . v of the autograd restatement against (y_s(x + h v) - y_s(x - h v)) / 2h of the independent torch_ref graph, in
    fp64, for random directions v over every input (structures are independent: one direction perturbs all of them, and each
    structure's derivative is read off its own output)."""
    import input_grad_ref
    import torch_ref

    cfg, w, _, pk = make_batch(**FD_CASES[case])
    y, grads = input_grad_ref.input_grads(cfg, w, pk)
    y0, _ = torch_ref.forward_packed(cfg, w, _as64(pk))
    assert np.allclose(y, y0.ravel(), rtol=1e-12, atol=1e-12)
    assert set(grads) == {"neighbor_distance", "neighbor_weight"} | ({"ring_aromatic"} if cfg["model"]["use_ring"] else set()) | \
        ({"atomic"} if cfg["model"]["feature"] == "cgcnn" else set())
    rng = np.random.default_rng(7)
    seg_e = np.repeat(np.repeat(np.arange(pk.n_struct), np.diff(pk.mol_offset)), np.diff(pk.edge_offset))
    seg_a = np.repeat(np.arange(pk.n_struct), np.diff(pk.mol_offset))
    h = 1e-5
    for name, g in grads.items():
        seg = seg_e if name in ("neighbor_distance", "neighbor_weight") else seg_a
        x = getattr(_as64(pk), FIELD[name])
        assert np.abs(g).max() > 0, name
        for _ in range(3):
            v = rng.standard_normal(x.shape)
            yp, _ = torch_ref.forward_packed(cfg, w, _as64(pk, **{FIELD[name]: x + h * v}))
            ym, _ = torch_ref.forward_packed(cfg, w, _as64(pk, **{FIELD[name]: x - h * v}))
            fd = (yp.ravel() - ym.ravel()) / (2 * h)
            gv = g * v if g.ndim == 1 else (g * v).sum(1)
            an = np.bincount(seg, weights=gv, minlength=pk.n_struct)
            scale = max(np.abs(an).max(), 1e-3)
            assert np.abs(fd - an).max() <= 1e-6 * scale, (name, fd, an)


# ---- the Python layer, against a stand-in engine ----

class _StandIn:
    """Engine stand-in: 'gradients' that are plain functions of each packed input, so that slicing and re-padding can be checked."""

    def __init__(self):
        self.uploads = 0

    def num_streams(self):
        return 2

    def upload(self, packed):
        self.uploads += 1
        return types.SimpleNamespace(packed=packed, free=lambda: None, release=lambda: None)

    def input_grads(self, rb, distance=True, weight=True, ring=False, cgcnn=False):
        p = rb.packed
        out = {"y": np.add.reduceat(np.r_[p.edge_dist, 0], p.edge_offset[p.mol_offset[:-1]]).astype(np.float32)}
        if distance:
            out["neighbor_distance"] = 2 * p.edge_dist + p.edge_weight
        if weight:
            out["neighbor_weight"] = 3 * p.edge_weight
        if ring:
            out["ring_aromatic"] = 5 * p.ring + 1
        if cgcnn:
            out["atomic"] = 7 * p.cgcnn + 1
        return out


def _model(cfg):
    return abi_checks.stand_in_model(cfg, lambda config: _StandIn(), ring=True)


@pytest.mark.parametrize("wrt,over", [(("neighbor_distanc",), {}), (("ring_aromatic",), {}), (("atomic",), {}),
                                      (("neighbor_weight", "global_attention"), {}), (("atomic",), dict(use_ring=True))])
def test_names_are_checked_before_anything_is_uploaded(wrt, over):
    cfg, _, inputs, pk = make_batch(**over)
    m = _model(cfg)
    for x in (inputs, pk):
        with pytest.raises(ValueError):
            m.input_gradients(x, wrt=wrt)
    assert m.engine.uploads == 0


def test_padded_results_are_repadded_with_zeros_in_masked_slots():
    from scann import _hip

    cfg, _, inputs, pk = make_batch(n=5, use_ring=True)
    m = _model(cfg)
    got = m.input_gradients(inputs, wrt=("neighbor_distance", "neighbor_weight", "ring_aromatic"))
    B, M, N = np.shape(inputs["neighbors"])
    amask = np.asarray(inputs["atom_mask"]).reshape(B, M) != 0
    em = (np.asarray(inputs["neighbor_mask"]) != 0) & amask[:, :, None]
    assert got["neighbor_distance"].shape == (B, M, N) and got["ring_aromatic"].shape == (B, M, 2)
    assert got["predict_property"].shape == (B, 1)
    assert (got["neighbor_distance"][~em] == 0).all() and (got["neighbor_weight"][~em] == 0).all()
    assert (got["ring_aromatic"][~amask] == 0).all()
    assert np.array_equal(got["neighbor_distance"][em], 2 * pk.edge_dist + pk.edge_weight)
    assert np.array_equal(got["neighbor_weight"], _hip.repad_edges(3 * pk.edge_weight, amask, inputs["neighbor_mask"]))
    assert np.array_equal(got["ring_aromatic"][amask], 5 * pk.ring + 1)
    d = np.asarray(inputs["neighbor_distance"], np.float32)
    assert np.allclose(got["predict_property"].ravel(), np.where(em, d, 0).sum((1, 2)), rtol=1e-6)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_batch_size_slices_match_one_call_per_slice(packed):
    from scann import _hip

    cfg, _, inputs, pk = make_batch(n=7, feature="cgcnn")
    wrt = ("neighbor_distance", "neighbor_weight", "atomic")
    m = _model(cfg)
    x = pk if packed else inputs
    whole = m.input_gradients(x, wrt=wrt, batch_size=3)
    assert m.engine.uploads == 3
    m.engine.uploads = 0
    per = []
    for s0 in range(0, 7, 3):
        if packed:
            per.append(m.input_gradients(_hip.slice_packed(pk, s0, min(s0 + 3, 7)), wrt=wrt, batch_size=100))
        else:
            per.append(m.input_gradients({k: np.asarray(v)[s0:s0 + 3] for k, v in inputs.items()}, wrt=wrt, batch_size=100))
    assert m.engine.uploads == 3
    for k in wrt + ("predict_property",):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in per])), k
    one = m.input_gradients(x, wrt=wrt, batch_size=7)
    for k in wrt + ("predict_property",):
        assert np.array_equal(whole[k], one[k]), k
    if packed:
        assert whole["neighbor_distance"].shape == (pk.n_edge,) and whole["atomic"].shape == (pk.n_atom, 92)


def test_scann_facade_scales_by_target_std():
    from scann.models.scann_model import SCANN

    cfg, _, inputs, _ = make_batch(n=3)
    s = SCANN.__new__(SCANN)
    s.model = _model(cfg)
    s.mean, s.std = 2.0, 0.5
    raw = s.model.input_gradients(inputs)
    got = s.input_gradients(inputs)
    assert np.array_equal(got["neighbor_distance"], raw["neighbor_distance"] * 0.5)
    assert np.array_equal(got["predict_property"], raw["predict_property"] * 0.5 + 2.0)


def test_input_gradient_kernels_use_no_scratch(hip_lib):
    """The three leaves of the data-gradient backward (csrc/scann_input_grad.hip) spill nothing, read from the built library's
    kernel descriptors."""
    from scann import _hip

    kern = {n: v for n, v in abi_checks.device_kernels(_hip.LIB_PATH).items() if "input_grad_kernel" in n}
    assert len(kern) == 3, sorted(kern)
    for name, (scratch, vgpr) in kern.items():
        assert scratch == 0, (name, scratch, vgpr)

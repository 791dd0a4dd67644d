"""GPU tests of the input gradients (scann_input_grads / HipModel.input_gradients): d y_s / d input against the fp64 autograd
restatement of tests/input_grad_ref.py, under the rule of test_gpu_training.check_grads (error <= max(floor, slack x the same graph's
torch-fp32 error), capped), and the call's promises: bit-reproducible, structures independent, nothing of the handle changed."""
import numpy as np
import pytest

import scann_oracle as so

pytestmark = pytest.mark.gpu

GRAD_FLOOR, GRAD_SLACK, GRAD_CAP = 2e-5, 4.0, 2e-4  # test_gpu_training.py's rule


def setup(n=6, L=2, seed=1, target=None, data=None, **over):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if target:
        cfg["hyper"]["target"] = target
    ring, cg = bool(cfg["model"]["use_ring"]), cfg["model"]["feature"] == "cgcnn"
    w = so.init_weights(cfg, 3, perturb=True)
    de, dn = data if data is not None else so.synth_dataset(n, seed, use_ring=ring)
    inputs, _ = so.pad_batch(de, dn, cfg["model"]["g_update"], use_ring=ring)
    if cg:
        inputs["atomic"] = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")[inputs["atomic"]]
    pk = _hip.pack_inputs(inputs)
    return cfg, w, inputs, pk, HipModel(cfg, w, device=0, infer=True)


def wrt_of(cfg):
    return ("neighbor_distance", "neighbor_weight") + (("ring_aromatic",) if cfg["model"]["use_ring"] else ()) + \
        (("atomic",) if cfg["model"]["feature"] == "cgcnn" else ())


def errors(got, ref):
    out = {}
    for k, r in ref.items():
        scale = max(float(np.sqrt(np.mean(r * r))), 1e-12)
        out[k] = float(np.max(np.abs(np.asarray(got[k], np.float64) - r)) / max(float(np.abs(r).max()), scale))
    return out


EDGE_LEAVES = ("neighbor_distance", "neighbor_weight")  # [n_edge]; every other leaf has one row per atom


def structure_errors(got, ref, pk):
    """errors() per structure: {leaf: [n_struct]}, each structure's worst entry over ITS OWN max |ref| (errors()' normalisation; the
    max dominates the rms), so that a structure with small gradients is not measured against the batch's largest.  A structure
    without entries in a leaf (no edges) counts as equal"""
    mol = pk.mol_offset.astype(np.int64)
    bounds = {True: pk.edge_offset.astype(np.int64)[mol], False: mol}

    def seg_max(x, b):
        out, full = np.zeros(len(b) - 1), b[1:] > b[:-1]
        if full.any():
            out[full] = np.maximum.reduceat(x, b[:-1][full])  # (the empty segments between two full ones have no rows to skip)
        return out

    out = {}
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        d = np.abs(np.asarray(got[k], np.float64) - r).reshape(r.shape[0], -1).max(1)
        b = bounds[k in EDGE_LEAVES]
        assert b[-1] == r.shape[0], (k, r.shape)
        out[k] = seg_max(d, b) / np.maximum(seg_max(np.abs(r).reshape(r.shape[0], -1).max(1), b), 1e-12)
    return out


def check(got, cfg, w, pk, refs=None, g32=None):
    """`g32`: the torch-fp32 graph's gradients where the caller has them already (the same call, made once)"""
    import input_grad_ref

    y64, ref = refs if refs is not None else input_grad_ref.input_grads(cfg, w, pk)
    if g32 is None:
        _, g32 = input_grad_ref.input_grads(cfg, w, pk, dtype="float32")
    e_gpu, e_32 = errors(got, ref), errors(g32, ref)
    bad = {k: (e_gpu[k], e_32[k]) for k in ref if not e_gpu[k] <= min(GRAD_CAP, max(GRAD_FLOOR, GRAD_SLACK * e_32[k]))}
    assert not bad, bad
    scale = max(float(np.sqrt(np.mean(y64 ** 2))), 1e-6)
    assert np.max(np.abs(got["predict_property"].ravel() - y64)) <= 1e-4 * scale
    return e_gpu


CASES = {
    "g_update_L2": dict(L=2),
    "g_update_L7": dict(L=7),
    "base_L2": dict(L=2, g_update=False),
    "base_L7": dict(L=7, g_update=False),
    "no_ga_norm": dict(use_ga_norm=False),
    "no_attn_norm": dict(use_attn_norm=False),
    "base_no_norms": dict(g_update=False, use_attn_norm=False, use_ga_norm=False),
    "ring": dict(use_ring=True),
    "cgcnn": dict(feature="cgcnn"),
    "ring_cgcnn_base": dict(use_ring=True, feature="cgcnn", g_update=False),
    "e_b": dict(target="e_b"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_input_gradients_match_autograd(hip_lib, case):
    cfg, w, _, pk, model = setup(**CASES[case])
    check(model.input_gradients(pk, wrt=wrt_of(cfg)), cfg, w, pk)


@pytest.mark.parametrize("case", ["64x4", "128x8"])
def test_input_gradients_on_the_plain_fp32_kernels(hip_lib, monkeypatch, case):
    """SCANN_GENERIC=1: the same leaves on the generic-width backward (64 / 4 only runs there; 128 / 8 is forced onto it)."""
    monkeypatch.setenv("SCANN_GENERIC", "1")
    over = dict(local_dim=64, num_head=4, global_dim=96, dense_out=32) if case == "64x4" else {}
    for extra in ({}, dict(g_update=False, use_ring=True), dict(feature="cgcnn")):
        cfg, w, _, pk, model = setup(**over, **extra)
        check(model.input_gradients(pk, wrt=wrt_of(cfg)), cfg, w, pk)


def test_input_gradients_with_more_than_64_neighbours(hip_lib):
    rng = np.random.default_rng(4)
    A = 140
    deg = {0: 70, 5: 130, 139: 65}
    nb = []
    for a in range(A):
        d = deg.get(a, int(rng.integers(1, 7)))
        js = rng.choice(np.delete(np.arange(A), a), d, replace=False)
        nb.append([[6, int(j), float(rng.uniform(0.4, 3.5)), float(rng.uniform(0.1, 1.0)), float(rng.uniform(0.9, 4.0))] for j in js])
    de, dn = so.synth_dataset(2, 3)
    de3, dn3 = np.empty(3, dtype=object), np.empty(3, dtype=object)
    de3[0], dn3[0] = de[0], dn[0]
    de3[1], dn3[1] = [[int(z) for z in rng.choice([1, 6, 7, 8], A)], 0.3], nb
    de3[2], dn3[2] = de[1], dn[1]
    for g_update in (True, False):
        cfg, w, _, pk, model = setup(data=(de3, dn3), g_update=g_update)
        check(model.input_gradients(pk), cfg, w, pk)


def test_input_gradients_on_a_large_batch(hip_lib):
    """mp2018-shaped batch of 128 crystals (~43 k edges, up to 24 neighbours): past the 32-row tile plan and the fused attention
    backward (tests/size_batches.py)."""
    import size_batches as sb

    cfg, w, _, pk, model = setup(data=sb.mp2018_b128_data(), L=2, n_atoms=95)
    assert pk.n_edge > sb.EDGE_TILE_32_MAX_EDGES
    check(model.input_gradients(pk, batch_size=pk.n_struct), cfg, w, pk)


def test_a_structure_alone_matches_it_inside_a_mixed_batch(hip_lib):
    from scann import _hip

    cfg, w, _, pk, model = setup(n=8)
    whole = model.input_gradients(pk)
    import input_grad_ref

    for s in (0, 5):
        one = _hip.slice_packed(pk, s, s + 1)
        alone = model.input_gradients(one)
        e0, e1 = pk.edge_offset[pk.mol_offset[s]], pk.edge_offset[pk.mol_offset[s + 1]]
        part = {k: whole[k][e0:e1] for k in ("neighbor_distance", "neighbor_weight")}
        part["predict_property"] = whole["predict_property"][s:s + 1]
        refs = input_grad_ref.input_grads(cfg, w, one)
        e_mixed = check(part, cfg, w, one, refs)
        e_alone = check(alone, cfg, w, one, refs)
        for k in e_mixed:
            assert errors(part, {k: np.asarray(alone[k], np.float64)})[k] <= max(GRAD_FLOOR, 2 * max(e_mixed[k], e_alone[k])), k


def test_two_calls_return_identical_bits(hip_lib):
    for over in ({}, dict(g_update=False, use_ring=True)):
        cfg, w, inputs, pk, model = setup(n=8, **over)
        a = model.input_gradients(inputs, wrt=wrt_of(cfg))
        b = model.input_gradients(inputs, wrt=wrt_of(cfg))
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_inference_handle_predicts_the_same_bits_afterwards(hip_lib):
    """predict (device packing of padded inputs, host packing of a PackedBatch, and the resident pipeline's outputs) is bit-identical
    before and after an input_gradients call on the same inference handle."""
    cfg, w, inputs, pk, model = setup(n=8)

    def run():
        y_pad, ga_pad = model.predict(inputs)
        y_pk, ga_pk = model.predict(pk)
        outs = model.predict(inputs, outputs=["predict_property", "local_attention_1", "after_Lc"])
        return [y_pad, ga_pad, y_pk, ga_pk] + list(outs)

    before = run()
    g = model.input_gradients(inputs)
    assert np.abs(g["neighbor_distance"]).max() > 0
    after = run()
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_training_state_is_untouched(hip_lib):
    """On a handle in training mode: gradients, weights and the next training step are bit-identical to a twin handle's that never
    called input_grads (Adam moments and the step counter enter the next step's weights).  Both in the deterministic training mode,
    whose steps are bit-reproducible."""
    from scann.models.scann_model import HipModel

    cfg, w, _, pk, _ = setup(n=8)
    targets = np.linspace(-1, 1, pk.n_struct).astype(np.float32)
    a, b = HipModel(cfg, w, device=0, deterministic=True), HipModel(cfg, w, device=0, deterministic=True)
    res = []
    for i, m in enumerate((a, b)):
        eng = m.engine
        eng.train_begin()
        rb = eng.upload(pk)
        eng.train_step(rb, targets, 1e-3, dropout=0.1, seed=3)
        sse = eng.train_forward(rb, targets, dropout=0.1, seed=4)
        eng.zero_grads()
        eng.train_backward(rb, sse, pk.n_struct)
        if i == 0:
            g = eng.input_grads(rb)
            assert np.abs(g["neighbor_distance"]).max() > 0
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


def test_a_training_handle_uses_its_current_weights(hip_lib):
    """after an optimiser step the gradients are those of the updated weights"""
    import input_grad_ref

    cfg, w, _, pk, _ = setup(n=6)
    from scann.models.scann_model import HipModel

    m = HipModel(cfg, w, device=0)
    eng = m.engine
    eng.train_begin()
    rb = eng.upload(pk)
    eng.train_step(rb, np.zeros(pk.n_struct, np.float32), 1e-2)
    w1 = eng.get_weights()
    got = eng.input_grads(rb)
    rb.free()
    got["predict_property"] = got.pop("y")
    y64, ref = input_grad_ref.input_grads(cfg, w1, pk)
    check(got, cfg, w1, pk, (y64, ref))


def test_weights_exact_checkpoint_is_refused(hip_lib):
    from scann import _hip

    cfg, w, _, pk, _ = setup(n=4)
    w = dict(w)
    k = w["local_attention_0/query/kernel"].copy()
    k[3, 5] = 300.0
    w["local_attention_0/query/kernel"] = k
    from scann.models.scann_model import HipModel

    model = HipModel(cfg, w, device=0, infer=True)
    with pytest.raises(_hip.ScannHipError) as ei:
        model.input_gradients(pk)
    assert ei.value.code == -2 and "255.9" in ei.value.detail  # SCANN_ERR_UNSUPPORTED (include/scann_hip.h)
    y = model.predict(pk)[0]
    assert np.isfinite(y).all()

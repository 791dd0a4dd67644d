"""GPU tests of the attention rollout (scann_attention_rollout through Engine.attention_rollout and HipModel.attention_rollout).

1. Kernel arithmetic, derived bound: the GPU's rollout / attribution against tests/rollout_ref.py in fp64 applied to the GPU's OWN maps
   (predict(outputs=[local_attention_<k>])) and its own GlobalAttention scores.  All terms are non-negative, so rounding errors do not
   amplify: per layer at most H roundings in the head mean, N_max in the products and the row sum, 4 in the mix, hence
   |got - ref| <= 2 * depth * (H + N_max + 4) * 2^-24 * ref entrywise (rollout_ref.kernel_bound; factor 2 for second-order terms and an
   unfused multiply-add), plus (n + 1) * 2^-24 relative for the attribution; entries below 1e-30 are compared absolutely.
2. End to end against the fp64 oracle: rel_err(gpu, fp64) <= max(1e-4, 2 * rel_err(fp32 oracle rollout, fp64)), rel_err and bound as
   tests/test_gpu_outputs.py has them for the maps themselves.
3. - 7.  y / ga bitwise the forward's, row sums, bitwise invariances, handle and batch state, limits, the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of the environment-switch test
    for p in (os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, p)

import rollout_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import _bits, rel_err, steady_memory, training_twin  # noqa: E402,F401

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def big220_data():
    """a 220-atom structure with atoms of 65 .. 219 neighbours (chunk tiles; several column slabs) between two small molecules, built
    as in test_gpu_outputs.py::test_outputs_of_atoms_with_more_than_64_neighbours"""
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
    return de3, dn3


def setup(kind="qm9", n=24, seed=0, L=None, data=None, isolate=False, infer=True, **over):
    from scann.models.scann_model import HipModel

    cfg = so.default_config(kind)
    if L is not None:
        cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    w = so.init_weights(cfg, 1234, perturb=True)
    if data == "big220":
        data = big220_data()
    de, dn = data if data is not None else so.synth_dataset(n, seed, kind=kind)
    inputs, _ = so.pad_batch(de, dn, g_update=cfg["model"]["g_update"])
    inputs = {k: np.array(v) for k, v in inputs.items()}
    if isolate:  # an isolated real atom
        real = np.nonzero(np.asarray(inputs["atom_mask"]).reshape(inputs["neighbor_mask"].shape[:2])[3])[0]
        inputs["neighbor_mask"][3, real[min(2, len(real) - 1)], :] = False
    return cfg, w, inputs, HipModel(cfg, w, device=0, infer=infer)


def gpu_maps(model, cfg, inputs):
    return model.predict(inputs, outputs=["local_attention_%d" % k for k in range(cfg["model"]["n_attention"])])


def check_kernel(got, cfg, inputs, maps, label, **kw):
    """bound 1 on a result of HipModel.attention_rollout (padded), the maps being the GPU's own; prints the figures before it asserts"""
    amask, em = rollout_ref.masks(inputs)
    depth = kw.get("depth") or cfg["model"]["n_attention"]
    bnd = rollout_ref.kernel_bound(depth, cfg["model"]["num_head"], int(em.sum(-1).max()))
    R64, a64 = rollout_ref.rollout(inputs, maps, got["global_attention"], dtype=np.float64, **kw)
    R = got["rollout"].astype(np.float64)
    assert R.shape == R64.shape and got["rollout"].dtype == np.float32
    assert np.array_equal(R != 0, R64 != 0) or np.all(np.abs(R - R64)[(R != 0) != (R64 != 0)] <= bnd * 1e-30)
    eR = float(np.max(np.abs(R - R64) / np.maximum(R64, 1e-30)))
    n_of = amask.sum(1)[:, None, None]
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(a64)
        assert np.array_equal(np.isfinite(got["atom_attribution"]), fin)
        tolA = (bnd + (n_of + 1) * EPS) * np.maximum(a64, 1e-30)
        ratioA = float(np.max((np.abs(got["atom_attribution"].astype(np.float64) - a64) / tolA)[fin]))
    print("%s: rollout max relative error %.3e (bound %.3e), attribution error / its bound %.3f" % (label, eR, bnd, ratioA))
    assert eR <= bnd, (label, eR, bnd)
    assert ratioA <= 1.0, (label, ratioA)
    return eR, bnd


KERNEL_CASES = {
    "qm9_isolated": (dict(isolate=True), dict()),
    "base": (dict(n=12, seed=3, g_update=False), dict()),
    "L1": (dict(n=12, seed=3, L=1), dict()),
    "no_attn_norm": (dict(n=12, seed=3, use_attn_norm=False), dict()),
    "mp2018": (dict(kind="mp2018", n=16, seed=1), dict()),
    "big220": (dict(data="big220"), dict()),
    "widths_64_4": (dict(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=32), dict()),
    "head3": (dict(), dict(head=3)),
    "depth2": (dict(), dict(depth=2)),
    "residual0": (dict(), dict(residual=0.0)),
    "residual025": (dict(), dict(residual=0.25)),
    "residual1": (dict(), dict(residual=1.0)),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_arithmetic_within_the_derived_bound(hip_lib, case):
    mk, kw = KERNEL_CASES[case]
    cfg, w, inputs, model = setup(**mk)
    got = model.attention_rollout(inputs, **kw)
    check_kernel(got, cfg, inputs, gpu_maps(model, cfg, inputs), case, **kw)
    if case == "big220":
        from scann import _hip

        rb = model.engine.upload(_hip.pack_inputs(inputs))
        assert model.engine.batch_info(rb)["big_atoms"] == 6
        rb.free()
    if case == "residual1":
        amask, _ = rollout_ref.masks(inputs)
        for b in range(len(amask)):
            assert np.array_equal(got["rollout"][b], np.diag(amask[b].astype(np.float32)))
        assert np.array_equal(got["atom_attribution"], got["global_attention"])


def test_kernel_arithmetic_under_scann_exact(hip_lib, tmp_path):
    """a handle whose forwards run on the exact-fp32 kernels (SCANN_EXACT=1, a fresh process)"""
    cfg, w, inputs, _ = setup(isolate=True)
    e = dict(os.environ)
    e["SCANN_EXACT"] = "1"
    out = tmp_path / "exact.npz"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    got = {k: z[k] for k in ("rollout", "atom_attribution", "global_attention", "predict_property")}
    check_kernel(got, cfg, inputs, [z["map_%d" % k] for k in range(cfg["model"]["n_attention"])], "SCANN_EXACT=1")


@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_end_to_end_against_the_fp64_oracle(hip_lib, kind):
    cfg, w, inputs, model = setup(kind=kind, n=16, seed=1, isolate=True)
    got = model.attention_rollout(inputs)
    ref = {}
    for dt in (np.float64, np.float32):
        inter = {}
        _, ga = so.forward(cfg, w, inputs, dt, intermediates=inter)
        maps = [inter["attn_local_%d" % (k + 1)] for k in range(cfg["model"]["n_attention"])]
        ref[dt] = rollout_ref.rollout(inputs, maps, ga, dtype=dt)
    amask, _ = rollout_ref.masks(inputs)
    for name, i, sel in (("rollout", 0, slice(None)), ("atom_attribution", 1, amask)):
        e_gpu, e_32 = rel_err(got[name][sel], ref[np.float64][i][sel]), rel_err(ref[np.float32][i][sel], ref[np.float64][i][sel])
        print("%s %s: gpu %.3e  fp32 oracle %.3e (both against the fp64 oracle)" % (kind, name, e_gpu, e_32))
        assert e_gpu <= max(1e-4, 2 * e_32), (name, e_gpu, e_32)


@pytest.mark.parametrize("mk", [dict(isolate=True), dict(kind="mp2018", n=16, seed=1), dict(n=12, seed=3, g_update=False)], ids=["qm9", "mp2018", "base"])
def test_y_and_ga_are_the_forwards_and_rows_sum_to_one(hip_lib, mk):
    cfg, w, inputs, model = setup(**mk)
    y, ga = model.predict(inputs)
    for kw in (dict(), dict(depth=2), dict(head=1, residual=0.1)):
        got = model.attention_rollout(inputs, **kw)
        assert np.array_equal(got["predict_property"].view(np.uint32), y.view(np.uint32))
        assert np.array_equal(got["global_attention"].view(np.uint32), ga.view(np.uint32))
        amask, em = rollout_ref.masks(inputs)
        depth = kw.get("depth") or cfg["model"]["n_attention"]
        bnd = 2 * depth * (int(em.sum(-1).max()) + 4) * EPS
        dev = float(np.max(np.abs(got["rollout"].astype(np.float64).sum(-1)[amask] - 1.0)))
        print("row sums of the rollout: max |sum - 1| = %.3e (bound %.3e)" % (dev, bnd))
        assert dev <= bnd
        assert not got["rollout"][~amask].any() and not got["rollout"].transpose(0, 2, 1)[~amask].any()
        s = got["atom_attribution"].astype(np.float64)[..., 0].sum(1)
        assert np.max(np.abs(s - ga.astype(np.float64)[..., 0].sum(1))) <= bnd + (amask.sum(1).max() + 1) * EPS


@pytest.mark.parametrize("mk", [dict(n=8), dict(n=8, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=32), dict(data="big220")],
                         ids=["qm9", "generic", "big220"])
def test_bitwise_repeat_alone_permuted_matrix_and_packed(hip_lib, mk):
    from scann import _hip

    cfg, w, inputs, model = setup(**mk)
    pk = _hip.pack_inputs(inputs)
    pk = _hip.PackedBatch(pk.atomic, pk.mol_offset, pk.edge_offset, pk.edge_col, pk.edge_dist, pk.edge_weight)
    a, b = model.attention_rollout(pk), model.attention_rollout(pk)
    for k in a:
        assert np.array_equal(_bits(a[k]) if a[k].dtype == np.float32 else a[k], _bits(b[k]) if b[k].dtype == np.float32 else b[k]), k
    B = pk.n_struct
    cnt = np.diff(pk.mol_offset).astype(np.int64)
    assert np.array_equal(a["rollout_offset"], np.concatenate([[0], np.cumsum(cnt * cnt)]))
    # matrix=False: the same attribution bits
    nm = model.attention_rollout(pk, matrix=False)
    assert "rollout" not in nm and np.array_equal(_bits(nm["atom_attribution"]), _bits(a["atom_attribution"]))
    # the padded dict: the same numbers at the padded positions
    pad = model.attention_rollout(inputs)
    amask, _ = rollout_ref.masks(inputs)
    assert np.array_equal(_bits(pad["atom_attribution"][amask][:, 0]), _bits(a["atom_attribution"]))
    assert np.array_equal(_bits(pad["global_attention"][amask][:, 0]), _bits(a["global_attention"]))
    for s in range(B):
        blk = a["rollout"][a["rollout_offset"][s]:a["rollout_offset"][s + 1]].reshape(cnt[s], cnt[s])
        assert np.array_equal(_bits(pad["rollout"][s][np.ix_(amask[s], amask[s])]), _bits(blk)), s
    # a structure alone (another column-slab width for the small neighbours of the 220-atom one) and in a permuted batch
    perm = np.random.default_rng(2).permutation(B)
    p = model.attention_rollout(_hip.pack_inputs({k: np.asarray(v)[perm] for k, v in inputs.items()}))
    for j, s in enumerate(perm):
        one = model.attention_rollout(_hip.slice_packed(pk, int(s), int(s) + 1))
        o0, o1, q0, q1 = pk.mol_offset[s], pk.mol_offset[s + 1], p["rollout_offset"][j], p["rollout_offset"][j + 1]
        r0, r1 = a["rollout_offset"][s], a["rollout_offset"][s + 1]
        assert np.array_equal(_bits(a["rollout"][r0:r1]), _bits(one["rollout"])), s
        assert np.array_equal(_bits(a["rollout"][r0:r1]), _bits(p["rollout"][q0:q1])), s
        assert np.array_equal(_bits(a["atom_attribution"][o0:o1]), _bits(one["atom_attribution"])), s
        assert a["predict_property"][s, 0].view(np.uint32) == one["predict_property"][0, 0].view(np.uint32) == p["predict_property"][j, 0].view(np.uint32)


def test_selected_outputs_and_the_batchs_output_block(hip_lib):
    """the handle's own selection survives the call, also a failing one; the batch's output block holds the maps the rollout was made from"""
    import ctypes as C

    from scann import _hip

    cfg, w, inputs, model = setup(n=6, seed=1, L=3)
    eng = model.engine
    names = ["local_attention_1", "after_Lc"]
    before = model.predict(inputs, outputs=names)
    map0 = model.predict(_hip.pack_inputs(inputs), outputs=["local_attention_0"])[0]
    eng.set_outputs([1], after_lc=True)
    try:
        rb = eng.upload(_hip.pack_inputs(inputs))
        eng.forward_resident(rb)
        eng.download(rb)
        sel0 = [eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 1), eng.read_output(rb, _hip.OUT_AFTER_LC)]
        with pytest.raises(_hip.ScannHipError):
            eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 0)
        assert eng.lib.scann_rollout_floats(eng._h, rb._h) == int((np.diff(rb.packed.mol_offset).astype(np.int64) ** 2).sum())
        got = eng.attention_rollout(rb)
        # right after the call the block belongs to the call's forward: layers 0 .. 2 and the handle's after_Lc
        assert np.array_equal(_bits(eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 0)), _bits(map0))
        assert np.array_equal(_bits(eng.read_output(rb, _hip.OUT_AFTER_LC)), _bits(sel0[1]))
        # failing calls: depth too large, bad residual / head (SCANN_ERR_INVALID through the C call)
        y = np.empty(rb.packed.n_struct, np.float32)
        call = lambda res, head, depth: eng.lib.scann_attention_rollout(eng._h, rb._h, C.c_float(res), head, depth, _hip._ptr(y), None, None, None)  # noqa: E731
        assert call(0.5, -1, 4) == -1 and call(-0.01, -1, 0) == -1 and call(1.5, -1, 0) == -1 and call(float("nan"), -1, 0) == -1
        assert call(float("inf"), -1, 0) == -1 and call(0.5, 8, 0) == -1 and call(0.5, -2, 0) == -1
        assert call(0.5, -1, 0) == 0 and call(0.5, 7, 3) == 0 and call(1.0, 0, 1) == 0  # every output pointer but y NULL
        assert np.array_equal(_bits(y), _bits(got["y"]))
        # the next forward writes the handle's own selection again
        eng.forward_resident(rb)
        eng.download(rb)
        assert np.array_equal(_bits(eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 1)), _bits(sel0[0]))
        assert np.array_equal(_bits(eng.read_output(rb, _hip.OUT_AFTER_LC)), _bits(sel0[1]))
        with pytest.raises(_hip.ScannHipError):
            eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 0)
        rb.free()
    finally:
        eng.set_outputs()
    model.attention_rollout(inputs)
    after = model.predict(inputs, outputs=names)
    assert all(np.array_equal(_bits(x), _bits(y_)) for x, y_ in zip(before, after))
    y0, ga0 = model.predict(inputs)
    assert np.array_equal(_bits(y0[:, 0]), _bits(got["y"]))


def test_repeated_calls_do_not_eat_device_memory(hip_lib):
    from scann import _hip

    cfg, w, inputs, model = setup(n=40, seed=2)
    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(inputs))
    first = eng.attention_rollout(rb)

    def call(rep):
        r = eng.attention_rollout(rb, matrix=rep % 2 == 0)
        assert np.array_equal(_bits(r["attribution"]), _bits(first["attribution"]))

    steady_memory(eng, call, 50, 32 << 20)  # (the slack of test_repeated_predicts_with_outputs_do_not_eat_device_memory)
    rb.free()


def test_training_handle(hip_lib):
    """after two training steps: the result is an inference handle's with the same weights, and weights, gradients and the following
    (deterministic) step are those of a twin that never made the call"""
    from scann import _hip

    cfg, w, inputs, _ = setup(n=8, seed=5, L=2)

    def calls(train_model, rb, inference):
        got = train_model.engine.attention_rollout(rb)
        inf_model, rb2 = inference()
        ref = inf_model.engine.attention_rollout(rb2)
        for k in ("y", "ga", "attribution", "rollout"):
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), k

    training_twin(cfg, w, _hip.pack_inputs(inputs), calls)


def test_limit_on_atoms_per_structure(hip_lib):
    """a structure of SCANN_ROLLOUT_MAX_ATOMS atoms is computed and meets bound 1; one atom more is SCANN_ERR_UNSUPPORTED with a message
    naming the size and the limit, and leaves the handle's selection as it was"""
    import size_batches
    from scann import _hip

    lim = _hip.ROLLOUT_MAX_ATOMS
    cfg, w, inputs, model = setup(L=2, data=size_batches.giant_data(lim))
    got = model.attention_rollout(inputs)
    check_kernel(got, cfg, inputs, gpu_maps(model, cfg, inputs), "giant %d" % lim)
    cfg, w, inputs, model = setup(L=2, data=size_batches.giant_data(lim + 1))
    eng = model.engine
    eng.set_outputs([1])
    try:
        rb = eng.upload(_hip.pack_inputs(inputs))
        with pytest.raises(_hip.ScannHipError) as e:
            eng.attention_rollout(rb)
        assert e.value.code == -2 and str(lim) in str(e.value) and str(lim + 1) in str(e.value)
        eng.forward_resident(rb)
        eng.download(rb)
        eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 1)
        with pytest.raises(_hip.ScannHipError):
            eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 0)
        rb.free()
    finally:
        eng.set_outputs()


def test_a_batch_without_edges(hip_lib):
    cfg, w, inputs, model = setup(n=5, seed=7, L=2)
    inputs["neighbor_mask"][:] = False
    got = model.attention_rollout(inputs)
    amask, _ = rollout_ref.masks(inputs)
    for b in range(len(amask)):
        assert np.array_equal(got["rollout"][b], np.diag(amask[b].astype(np.float32)))
    assert np.array_equal(_bits(got["atom_attribution"]), _bits(got["global_attention"]))
    y, ga = model.predict(inputs)
    assert np.array_equal(_bits(got["predict_property"]), _bits(y)) and np.array_equal(_bits(got["global_attention"]), _bits(ga))


def test_python_layer_slices_and_denormalises(hip_lib):
    from scann.models.scann_model import SCANN

    cfg, w, inputs, model = setup(n=10, seed=5, L=2)
    one = model.attention_rollout(inputs, batch_size=64)
    cut = model.attention_rollout(inputs, batch_size=3)
    assert sorted(one) == sorted(cut) == ["atom_attribution", "global_attention", "predict_property", "rollout"]
    for k in one:
        assert np.array_equal(_bits(one[k]), _bits(cut[k])), k
    s = SCANN.__new__(SCANN)
    s.model, s.mean, s.std = model, 1.5, 0.25
    got = s.attention_rollout(inputs)
    assert np.array_equal(got["predict_property"], one["predict_property"] * 0.25 + 1.5)
    for k in ("global_attention", "atom_attribution", "rollout"):
        assert np.array_equal(_bits(got[k]), _bits(one[k])), k
    with pytest.raises(ValueError):
        model.attention_rollout(inputs, depth=3)


def test_cli_writes_the_rollout(hip_lib, tmp_path):
    """predict_model.py --rollout: rollout_<target>.pickle, one unpadded dict per structure; the other files' bytes are those of a run
    without the flag"""
    import yaml

    from scann.models import SCANN
    from scann.models.scann_model import save_container

    n = 20
    de, dn = so.synth_dataset(n, 5)
    full = np.empty(n, dtype=object)
    for i in range(n):
        full[i] = {"Atomic": de[i][0], "Properties": {"homo": float(i)}}
    np.save(tmp_path / "data_energy.npy", full, allow_pickle=True)
    np.save(tmp_path / "data_nei.npy", dn, allow_pickle=True)
    cfg = so.default_config("qm9")
    cfg["model"]["n_attention"] = 2
    cfg["hyper"].update(batch_size=8, scaler=False, use_ref=False, target="homo", data_energy_path=str(tmp_path / "data_energy.npy"),
                        data_nei_path=str(tmp_path / "data_nei.npy"), save_path=str(tmp_path / "run"))
    out = tmp_path / "model"
    os.makedirs(out / "models")
    yaml.safe_dump(cfg, open(out / "config.yaml", "w"))
    save_container(str(out / "models" / "model_homo.h5"), cfg, so.init_weights(cfg, 77, perturb=True))
    cli = [sys.executable, os.path.join(ROOT, "predict_model.py"), str(out)]
    r = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plain = {f: open(out / f, "rb").read() for f in ("ga_scores_homo.pickle", "energy_pre_homo.pickle")}
    assert not os.path.exists(out / "rollout_homo.pickle")
    r = subprocess.run(cli + ["--rollout", "--rollout-residual", "0.25"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    got = pickle.load(open(out / "rollout_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    i = 0
    for b in range(len(scann.dataIter)):
        inputs, _ = scann.dataIter[b]
        ref = scann.attention_rollout(inputs, residual=0.25)
        amask, _ = rollout_ref.masks(inputs)
        for s in range(len(amask)):
            d = got[i]
            assert sorted(d) == ["attribution", "rollout"]
            assert np.array_equal(d["attribution"], ref["atom_attribution"][s][amask[s], 0])
            assert np.array_equal(d["rollout"], ref["rollout"][s][np.ix_(amask[s], amask[s])])
            i += 1
    assert i == n == len(got)


if __name__ == "__main__":
    cfg_, w_, inputs_, model_ = setup(isolate=True)
    res_ = model_.attention_rollout(inputs_)
    for k_, m_ in enumerate(gpu_maps(model_, cfg_, inputs_)):
        res_["map_%d" % k_] = m_
    np.savez(sys.argv[1], **res_)

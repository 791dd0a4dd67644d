"""GPU tests of model sets (scann_models_load / scann_forward_models / ModelSet): every member bitwise equal to its own single-model
HipModel -- over the branch cases of the Monte Carlo tests, the tile switches of tests/size_batches.py, padded and packed inputs --,
permutation of the members, exact-fp32 members, the range-guard re-run, and what the set leaves untouched."""
import copy

import numpy as np
import pytest

import scann_oracle as so
import size_batches as sb
from test_gpu_mc_dropout import CASES
from test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu


def config(L=2, target=None, widths=None, kind="qm9", **over):
    cfg = so.default_config(kind)
    cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if widths:
        cfg["model"].update(widths)
        cfg["model"]["n_atoms"] = 100
    if target:
        cfg["hyper"]["target"] = target
    return cfg


def members(cfg, K, seed=3, targets=None):
    out = []
    for m in range(K):
        c = copy.deepcopy(cfg)
        if targets:
            c["hyper"]["target"] = targets[m]
        out.append((c, so.init_weights(c, seed + 17 * m, perturb=True)))
    return out


def inputs_of(cfg, n=6, seed=1):
    ring, cg = bool(cfg["model"]["use_ring"]), cfg["model"]["feature"] == "cgcnn"
    de, dn = so.synth_dataset(n, seed, use_ring=ring)
    inputs, _ = so.pad_batch(de, dn, cfg["model"]["g_update"], use_ring=ring)
    if cg:
        inputs["atomic"] = np.random.default_rng(5).integers(0, 2, size=(101, 92)).astype("float32")[inputs["atomic"]]
    return inputs


def singles(mem, inputs):
    from scann.models.scann_model import HipModel

    out = []
    for c, w in mem:
        y, ga = HipModel(c, w, device=0, infer=True).predict(inputs)
        out.append((y, ga))
    return out


def assert_members_equal(got, ref):
    K = len(ref)
    assert got["predict_property"].shape[0] == K and got["global_attention"].shape[0] == K
    for m, (y, ga) in enumerate(ref):
        assert np.array_equal(got["predict_property"][m], y), (m, np.max(np.abs(got["predict_property"][m] - y)))
        assert np.array_equal(got["global_attention"][m], ga), m


@pytest.mark.parametrize("K", [1, 2, 5])
def test_members_bitwise_equal_their_single_models(hip_lib, K):
    from scann import _hip
    from scann.models import ModelSet

    cfg = config()
    mem = members(cfg, K)
    inputs = inputs_of(cfg)
    ref = singles(mem, inputs)
    ms = ModelSet(mem, device=0)
    assert ms.engine.models_count() == K
    assert_members_equal(ms.predict(inputs), ref)
    pk = _hip.pack_inputs(inputs)
    assert sb.upload_tile_rows(pk)[0] == 32  # (32-row edge tiles; test_tile_switches runs the 64-row plans)
    assert_members_equal(ms.predict(pk), ref)  # a PackedBatch of a padded dict: its scores come back padded
    got = ms.predict(pk, batch_size=4)  # in slices through the pipeline
    assert_members_equal(got, ref)
    # each member within the parity bound of the NumPy oracle
    for m, (c, w) in enumerate(mem):
        y_ref, ga_ref = so.forward(c, w, inputs, np.float32)
        assert rel_err(got["predict_property"][m], y_ref) <= RTOL and rel_err(got["global_attention"][m], ga_ref) <= RTOL


@pytest.mark.parametrize("case", list(CASES))
def test_branch_cases(hip_lib, case):
    from scann.models import ModelSet

    over = dict(CASES[case])
    cfg = config(**over)
    targets = None
    if case == "e_b":  # an e_b member (mrelu head) beside a member of another target in one set
        targets = ["e_b", "homo", "e_b"]
    mem = members(cfg, 3, targets=targets)
    inputs = inputs_of(cfg)
    assert_members_equal(ModelSet(mem, device=0).predict(inputs), singles(mem, inputs))


@pytest.mark.parametrize("name", ["mp2018_b128", "qm9_b260", "sparse_atoms"])
def test_tile_switches(hip_lib, name):
    """the batches of tests/size_batches.py that cross the tile switches, through a PackedBatch: 64-row edge tiles (all three; the small
    batches of the other tests plan 32-row ones), and -- sparse_atoms, 34 k atoms -- 64-row atom tiles, atom_kernel<.., RT = 2, .., SET>
    (launch_atom switches above 32,768 atoms per member)"""
    from scann.models import ModelSet
    from scann.models.scann_model import HipModel

    kind = "mp2018" if name.startswith("mp2018") else "qm9"
    cfg = config(kind=kind, L=so.default_config(kind)["model"]["n_attention"])
    pk, _ = getattr(sb, name)()
    assert sb.upload_tile_rows(pk)[0] == 64
    assert (pk.n_atom > 32 * 1024) == (name == "sparse_atoms")
    mem = members(cfg, 2)
    got = ModelSet(mem, device=0).predict(pk)
    for m, (c, w) in enumerate(mem):
        y, ga = HipModel(c, w, device=0, infer=True).engine.forward(pk)
        assert np.array_equal(got["predict_property"][m][:, 0], y)
        assert np.array_equal(got["global_attention"][m], pk.repad_ga(ga))


def test_more_than_64_neighbours(hip_lib):
    """chunk tiles + the softmax merge (edge_merge_kernel's set launch)"""
    from scann.models import ModelSet

    cfg = config()
    rng = np.random.default_rng(0)
    A = 70
    big = [[[6, int(j), float(rng.uniform(0.4, 3.5)), 1.0, float(rng.uniform(0.9, 4.0))]
            for j in rng.choice(np.delete(np.arange(A), a), 64, replace=False)] for a in range(A)]
    big[0].append([6, 1, 1.0, 1.0, 1.0])
    de, dn = so.synth_dataset(1, 3)
    de2, dn2 = np.empty(2, dtype=object), np.empty(2, dtype=object)
    de2[0], dn2[0] = [[6] * A, 0.0], big
    de2[1], dn2[1] = de[0], dn[0]
    inputs, _ = so.pad_batch(de2, dn2, True)
    mem = members(cfg, 3)
    assert_members_equal(ModelSet(mem, device=0).predict(inputs), singles(mem, inputs))


def test_permuting_members_permutes_outputs(hip_lib):
    from scann.models import ModelSet

    cfg = config()
    mem = members(cfg, 4)
    inputs = inputs_of(cfg, n=9)
    a = ModelSet(mem, device=0).predict(inputs)
    perm = [2, 0, 3, 1]
    b = ModelSet([mem[i] for i in perm], device=0).predict(inputs)
    for k in ("predict_property", "global_attention"):
        assert np.array_equal(b[k], a[k][perm])


def test_exact_member_runs_alone(hip_lib):
    """a member with a 128x128 weight of 300.0 runs on the exact-fp32 kernels and equals its single handle; the others are unchanged"""
    from scann.models import ModelSet

    cfg = config()
    mem = members(cfg, 3)
    inputs = inputs_of(cfg)
    plain = ModelSet(mem, device=0).predict(inputs)
    w = dict(mem[1][1])
    k = w["local_attention_0/query/kernel"].copy()
    k[3, 5] = 300.0
    w["local_attention_0/query/kernel"] = k
    mem[1] = (mem[1][0], w)
    got = ModelSet(mem, device=0).predict(inputs)
    assert_members_equal(got, singles(mem, inputs))
    for m in (0, 2):
        assert np.array_equal(got["predict_property"][m], plain["predict_property"][m])


def test_range_guard_reruns_every_member_exact(hip_lib, monkeypatch):
    from scann.models import ModelSet

    cfg = config(L=3)
    mem = members(cfg, 3)
    w = dict(mem[1][1])
    # (scaling residual_norm_2/dense_1/kernel by 3000 takes these weights past |w| = 255.9: that member would run exact from the start,
    #  test_exact_member_runs_alone; an activation beyond the split-fp16 range trips the guard, as in tests/test_gpu_outputs.py)
    w["after_Lc/bias"] = (w["after_Lc/bias"] + 1.0e5).astype(np.float32)
    mem[1] = (mem[1][0], w)
    inputs = inputs_of(cfg)
    ms = ModelSet(mem, device=0)
    assert ms.engine.exact_reruns() == 0
    got = ms.predict(inputs)
    assert ms.engine.exact_reruns() == 1
    monkeypatch.setenv("SCANN_EXACT", "1")
    assert_members_equal(got, singles(mem, inputs))


def test_set_leaves_the_handle_untouched(hip_lib):
    from scann import _hip
    from scann.models import ModelSet

    cfg = config()
    mem = members(cfg, 3)
    inputs = inputs_of(cfg)
    ms = ModelSet(mem, device=0)
    eng = ms.engine
    y0, ga0 = ms.model.predict(inputs)
    # the batch's last single-model y and the selected outputs survive a set forward on the same batch
    pk = _hip.pack_inputs(inputs)
    rb = eng.upload(pk)
    eng.set_outputs([0], after_lc=True)
    eng.forward_resident(rb, 0)
    z = eng.read_output(rb, _hip.OUT_AFTER_LC)
    eng.forward_models(rb, 1)
    ys, _ = eng.models_download(rb)
    y1, _ = eng.download(rb)
    assert np.array_equal(y1, y0[:, 0]) and np.array_equal(eng.read_output(rb, _hip.OUT_AFTER_LC), z)
    eng.set_outputs()
    rb.free()
    y2, ga2 = ms.model.predict(inputs)
    assert np.array_equal(y2, y0) and np.array_equal(ga2, ga0)
    # repeated set predicts of one shape do not take device memory
    ms.predict(inputs)
    free0, _ = eng.device_memory()
    for _ in range(5):
        ms.predict(inputs)
    free1, _ = eng.device_memory()
    assert free1 >= free0


def test_training_handle_untouched(hip_lib):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = config()
    mem = members(cfg, 2)
    inputs = inputs_of(cfg)
    model = HipModel(cfg, mem[0][1], device=0)
    eng = model.engine
    eng.train_begin()
    pk = _hip.pack_inputs(inputs)
    rb = eng.upload(pk)
    eng.train_forward(rb, np.zeros(pk.n_struct, np.float32))
    w0, g0 = eng.get_weights(), eng.get_grads()
    eng.models_load([w for _, w in mem])
    eng.forward_models(rb, 0)
    eng.models_download(rb)
    w1, g1 = eng.get_weights(), eng.get_grads()
    rb.free()
    for k in w0:
        assert np.array_equal(w0[k], w1[k]) and np.array_equal(g0[k], g1[k]), k


def test_forward_without_set_is_refused(hip_lib):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = config()
    model = HipModel(cfg, so.init_weights(cfg, 3), device=0, infer=True)
    rb = model.engine.upload(_hip.pack_inputs(inputs_of(cfg)))
    with pytest.raises(_hip.ScannHipError) as e:
        model.engine.forward_models(rb, 0)
    assert e.value.code == -5
    rb.free()


def test_download_belongs_to_the_current_set(hip_lib):
    """a download after another set was loaded (same K) is refused; two set forwards on two streams without a download in between
    write one workspace in order"""
    from scann import _hip
    from scann.models import ModelSet

    cfg = config()
    mem = members(cfg, 2)
    inputs = inputs_of(cfg)
    ref = singles(mem, inputs)
    ms = ModelSet(mem, device=0)
    eng = ms.engine
    rb = eng.upload(_hip.pack_inputs(inputs))
    eng.forward_models(rb, 0)
    eng.models_load([w for _, w in members(cfg, 2, seed=50)])
    with pytest.raises(_hip.ScannHipError) as e:
        eng.models_download(rb)
    assert e.value.code == -1
    eng.models_load([w for _, w in mem])
    eng.forward_models(rb, 0)
    eng.forward_models(rb, 1)
    y, ga = eng.models_download(rb)
    rb.free()
    for m, (y_ref, _) in enumerate(ref):
        assert np.array_equal(y[m], y_ref[:, 0])


def test_predict_model_with_writes_what_each_model_writes_alone(hip_lib, tmp_path):
    """predict_model.py <homo> --with <lumo> (lumo trained with hyper.scaler): each folder's pickles are bitwise the ones its own
    predict_model.py run writes"""
    import os
    import pickle
    import subprocess
    import sys

    from test_model_set_host import _trained_dirs

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dirs, _ = _trained_dirs(tmp_path, ["homo", "lumo"], scaler=(1,))
    files = [os.path.join(dirs[0], "energy_pre_homo.pickle"), os.path.join(dirs[0], "ga_scores_homo.pickle"),
             os.path.join(dirs[1], "energy_pre_lumo.pickle"), os.path.join(dirs[1], "ga_scores_lumo.pickle")]
    for d in dirs:
        r = subprocess.run([sys.executable, os.path.join(root, "predict_model.py"), d], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    alone = [pickle.load(open(f, "rb")) for f in files]
    for f in files:
        os.remove(f)
    r = subprocess.run([sys.executable, os.path.join(root, "predict_model.py"), dirs[0], "--with", dirs[1]], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, a in zip(files, alone):
        b = pickle.load(open(f, "rb"))
        if f.endswith(".pickle") and "energy_pre" in f:
            assert all(np.array_equal(np.asarray(x), np.asarray(z)) for x, z in zip(a, b)), f
        else:
            assert len(a) == len(b) and all(np.array_equal(x, z) and x.dtype == z.dtype for x, z in zip(a, b)), f

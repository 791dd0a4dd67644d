"""GPU tests of the per-atom contributions (scann_ablate_pooling through its ctypes binding Engine.ablate_pooling, and
HipModel.atom_contributions above it): the prediction with atoms left out of the global pooling against tests/ablate_ref.py -- the
oracle's after_Lc rows, then oracle.global_attention with the edited mask and the two head layers per kept set, fp32 and fp64.

Bound for `ablated`: rel_err(gpu, ref64) <= max(1e-4, 2 * rel_err(ref32, ref64)) over the finite entries of ref64 (1e-4: BASELINE.json's
north-star tolerance; 2: the slack of the parity tests), and the non-finite positions equal to the fp32 oracle's.  The ranking is the
GPU's own `order` (a near-tie cannot flip the comparison); `order` is checked on its own.

Bound for `contribution` (= y - ablated, a small difference of two predictions): measured in isolation from the upstream split-fp16
error -- the GPU's own after_Lc rows are the input of ablate_ref in fp32 and fp64 -- against the fp32 oracle's own error on the same rows:
rel_err(c_gpu, c64) <= CONTRIB_F * rel_err(c32, c64); see CONTRIB_F."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of the environment-switch tests
    for p in (os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, p)

import ablate_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from ablate_ref import MODES, rel_err  # noqa: E402
from analysis_checks import training_twin  # noqa: E402

pytestmark = pytest.mark.gpu

# twice the worst ratio rel_err(c_gpu, c64) / rel_err(c32, c64) over the fixtures of CASES, rounded up to an integer; the record is
# profiles/ablate_parity.txt (tools/ablate_parity.py writes it from contribution_errors below): ratios 0.54 - 1.12, the worst on the
# generic-width fixture (GPU 1.02e-4 against the fp32 oracle's 9.1e-5), 1.00 on the QM9 and MP2018 batches (2.9e-4 and 3.5e-4 on both sides)
CONTRIB_F = 3


def tiny_data():
    """structures of 1, 2, 3 and 5 atoms, every atom a neighbour of every other"""
    rng = np.random.default_rng(11)
    sizes = [1, 2, 3, 5]
    de, dn = np.empty(len(sizes), dtype=object), np.empty(len(sizes), dtype=object)
    for s, n in enumerate(sizes):
        Z = rng.choice([1, 6, 7, 8], n)
        nb = []
        for a in range(n):
            js = [j for j in range(n) if j != a]
            ang, dist = rng.uniform(0.4, 3.5, len(js)), rng.uniform(0.9, 4.0, len(js))
            nb.append([[int(Z[j]), int(j), float(ang[k]), float(ang[k] / ang.max()), float(dist[k])] for k, j in enumerate(js)])
        de[s], dn[s] = [[int(z) for z in Z], float(rng.normal())], nb
    return de, dn


CASES = {
    "qm9": dict(kind="qm9", n=32),
    "mp2018": dict(kind="mp2018", n=32),
    "no_ga_norm": dict(kind="qm9", n=8, L=2, use_ga_norm=False),
    "e_b": dict(kind="qm9", n=8, L=2, target="e_b"),
    "base": dict(kind="qm9", n=8, L=2, g_update=False),
    "generic": dict(kind="qm9", n=8, L=2, local_dim=64, num_head=4, global_dim=96, dense_out=80),
    "tiny": dict(kind="qm9", L=2, data="tiny"),
    "tiny_no_ga_norm": dict(kind="qm9", L=2, data="tiny", use_ga_norm=False),
}


def setup(kind="qm9", n=32, seed=5, L=None, target=None, data=None, infer=True, **over):
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg = so.default_config(kind)
    if L is not None:
        cfg["model"]["n_attention"] = L
    cfg["model"].update(over)
    if target:
        cfg["hyper"]["target"] = target
    w = so.init_weights(cfg, 3, perturb=True)
    if isinstance(data, str):
        data = tiny_data()
    de, dn = data if data is not None else so.synth_dataset(n, seed, kind=kind)
    inputs, _ = so.pad_batch(de, dn, g_update=cfg["model"]["g_update"])
    pk = _hip.pack_inputs(inputs)
    return cfg, w, inputs, pk, HipModel(cfg, w, device=0, infer=infer)


def run(model, pk, mode):
    rb = model.engine.upload(pk)
    try:
        return model.engine.ablate_pooling(rb, mode)
    finally:
        rb.free()


def references(cfg, w, inputs, mode, order):
    """ablate_ref on the oracle's own after_Lc rows: (ablated64, y64, ablated32, y32)"""
    out = []
    with np.errstate(all="ignore"):
        for dt in (np.float64, np.float32):
            z, mol = ablate_ref.after_lc(cfg, w, inputs, dt)
            out += list(ablate_ref.ablate(cfg, w, z, mol, mode, order, dt))
    return out


def check_against_reference(got, cfg, w, inputs, pk, mode, label):
    a64, y64, a32, y32 = references(cfg, w, inputs, mode, got["order"])
    ablate_ref.check_order(got["order"], got["ga"], pk.mol_offset)
    return ablate_ref.check_ablated(got["ablated"], a64, a32, "%s %s" % (label, mode)), (a64, y64, a32, y32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_modes_match_the_reference(hip_lib, case, mode):
    cfg, w, inputs, pk, model = setup(**CASES[case])
    eng = model.engine
    rb = eng.upload(pk)
    eng.forward_resident(rb)
    y_f, ga_f = eng.download(rb)
    got = eng.ablate_pooling(rb, mode)
    rb.free()
    # y and ga of the call are the forward's, bitwise (NaN bits included)
    assert np.array_equal(got["y"].view(np.uint32), y_f.view(np.uint32)) and np.array_equal(got["ga"].view(np.uint32), ga_f.view(np.uint32))
    (e_gpu, e_32), _ = check_against_reference(got, cfg, w, inputs, pk, mode, case)
    if mode == "insertion":  # k = n is the plain forward's quantity, in another summation order
        last = got["ablated"][pk.mol_offset[1:] - 1]
        assert np.array_equal(np.isnan(last), np.isnan(got["y"]))
        fin = np.isfinite(got["y"])
        e = rel_err(last[fin], got["y"][fin])
        print("insertion[k = n] against y: %.3e" % e)
        assert e <= max(1e-4, 2 * e_32)
    if case.startswith("tiny"):
        n_bad = int((~np.isfinite(got["ablated"])).sum())
        # with use_ga_norm a pooling over one atom or none is 0 / 0; structures of 1, 2, 3, 5 atoms
        want = {"leave_one_out": 1 + 2, "deletion": 1 + 2 + 2 + 2, "insertion": 1 + 1 + 1 + 1}[mode] if cfg["model"]["use_ga_norm"] else 0
        assert n_bad == want, (n_bad, want, got["ablated"])


def contribution_errors(case):
    """(rel_err(c_gpu, c64), rel_err(c32, c64)) of the leave-one-out contributions of one fixture, the GPU's own after_Lc rows as the
    reference's input (so the split-fp16 error upstream of the pooling is in neither figure)"""
    cfg, w, inputs, pk, model = setup(**CASES[case])
    got = run(model, pk, "leave_one_out")
    z = model.predict(pk, outputs=["after_Lc"])[0]
    with np.errstate(all="ignore"):
        a64, y64 = ablate_ref.ablate(cfg, w, z, pk.mol_offset, "leave_one_out", got["order"], np.float64)
        a32, y32 = ablate_ref.ablate(cfg, w, z, pk.mol_offset, "leave_one_out", got["order"], np.float32)
    cnt = np.diff(pk.mol_offset)
    c64 = np.repeat(y64, cnt) - a64
    c32 = np.repeat(y32, cnt) - a32  # fp32 arithmetic
    c_gpu = np.repeat(got["y"], cnt) - got["ablated"]
    fin = np.isfinite(c64)
    assert np.array_equal(~np.isfinite(c_gpu), ~np.isfinite(c32))
    return rel_err(c_gpu[fin], c64[fin]), rel_err(c32[fin], c64[fin])


@pytest.mark.parametrize("case", list(CASES))
def test_contributions_are_as_exact_as_the_fp32_oracle(hip_lib, case):
    e_gpu, e_32 = contribution_errors(case)
    print("contribution %s: gpu %.3e  fp32 oracle %.3e  ratio %.2f" % (case, e_gpu, e_32, e_gpu / max(e_32, 1e-30)))
    assert e_gpu <= CONTRIB_F * e_32, (e_gpu, e_32)


def _child(env, case, out):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, str(out)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out)


@pytest.mark.parametrize("case", ["qm9", "mp2018"])
def test_mfma_kernel_against_the_plain_fp32_one(hip_lib, tmp_path, case):
    """128 / 8 forced onto the generic-width kernels (SCANN_GENERIC=1, a fresh process): both implementations within the bound"""
    cfg, w, inputs, pk, model = setup(**CASES[case])
    gen = _child({"SCANN_GENERIC": "1"}, case, tmp_path / "gen.npz")
    for mode in MODES:
        got = run(model, pk, mode)
        check_against_reference(got, cfg, w, inputs, pk, mode, case + " mfma")
        g = {k: gen[mode + "_" + k] for k in ("y", "ga", "ablated", "order")}
        check_against_reference(g, cfg, w, inputs, pk, mode, case + " generic")


def test_exact_fp32_forward(hip_lib, tmp_path):
    """SCANN_EXACT=1 (a fresh process): the forward on the exact-fp32 kernels, the ablation consumes its gq / gk"""
    cfg, w, inputs, pk, model = setup(**CASES["qm9"])
    ex = _child({"SCANN_EXACT": "1"}, "qm9", tmp_path / "exact.npz")
    for mode in MODES:
        g = {k: ex[mode + "_" + k] for k in ("y", "ga", "ablated", "order")}
        check_against_reference(g, cfg, w, inputs, pk, mode, "exact")


@pytest.mark.parametrize("case", ["qm9", "generic"])
def test_bitwise_repeat_permutation_and_alone(hip_lib, case):
    from scann import _hip

    cfg, w, inputs, pk, model = setup(**dict(CASES[case], n=8))
    B = pk.n_struct
    perm = np.random.default_rng(2).permutation(B)
    inputs_p = {k: np.asarray(v)[perm] for k, v in inputs.items()}
    pk_p = _hip.pack_inputs(inputs_p)
    for mode in MODES:
        a, b = run(model, pk, mode), run(model, pk, mode)
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (mode, k)
        p = run(model, pk_p, mode)
        for j, s in enumerate(perm):
            o0, o1, q0, q1 = pk.mol_offset[s], pk.mol_offset[s + 1], pk_p.mol_offset[j], pk_p.mol_offset[j + 1]
            one = run(model, _hip.slice_packed(pk, int(s), int(s) + 1), mode)
            for k in ("ablated", "order", "ga"):
                assert np.array_equal(a[k][o0:o1].view(np.uint32), p[k][q0:q1].view(np.uint32)), (mode, k, s)
                assert np.array_equal(a[k][o0:o1].view(np.uint32), one[k].view(np.uint32)), (mode, k, s)
            assert a["y"][s].view(np.uint32) == p["y"][j].view(np.uint32) == one["y"][0].view(np.uint32)


def test_training_handle(hip_lib):
    """after two training steps: the result is an inference handle's with the same weights, and weights, gradients and the following
    (deterministic) step are those of a twin that never made the call"""
    cfg, w, inputs, pk, _ = setup(kind="qm9", n=8, L=2)

    def calls(train_model, rb, inference):
        got = {m: train_model.engine.ablate_pooling(rb, m) for m in MODES}
        inf, _ = inference()
        for m in MODES:
            ref = run(inf, pk, m)
            assert np.array_equal(got[m]["order"], ref["order"]), m
            for k in ("y", "ablated", "ga"):  # (the training handle's forward reads the same fp32 master weights' images)
                assert np.array_equal(got[m][k].view(np.uint32), ref[k].view(np.uint32)), (m, k)

    training_twin(cfg, w, pk, calls)


def test_unknown_mode_and_selected_outputs(hip_lib):
    from scann import _hip

    cfg, w, inputs, pk, model = setup(kind="qm9", n=4, L=2)
    eng = model.engine
    rb = eng.upload(pk)
    y = np.empty(pk.n_struct, np.float32)
    assert eng.lib.scann_ablate_pooling(eng._h, rb._h, 3, _hip._ptr(y), None, None, None) == -1  # SCANN_ERR_INVALID
    assert eng.lib.scann_ablate_pooling(eng._h, rb._h, 0, None, None, None, None) == 0  # every output pointer may be NULL
    rb.free()
    z0 = model.predict(inputs, outputs=["after_Lc"])[0]
    model.atom_contributions(inputs)
    assert np.array_equal(model.predict(inputs, outputs=["after_Lc"])[0], z0)


def test_python_layer_chunks_and_denormalisation(hip_lib):
    from scann.models.scann_model import SCANN

    cfg, w, inputs, pk, model = setup(kind="qm9", n=10, L=2)
    for mode in MODES:
        one = model.atom_contributions(inputs, mode=mode, batch_size=64)
        cut = model.atom_contributions(inputs, mode=mode, batch_size=3)
        assert sorted(one) == sorted(cut)
        for k in one:
            assert np.array_equal(one[k].view(np.uint32), cut[k].view(np.uint32)), (mode, k)
        raw = run(model, pk, mode)
        amask = np.asarray(inputs["atom_mask"]).reshape(one["order"].shape) != 0
        assert np.array_equal(one["ablated"][amask][:, 0].view(np.uint32), raw["ablated"].view(np.uint32))
        assert np.array_equal(one["y"][:, 0].view(np.uint32), raw["y"].view(np.uint32))
        y_p, ga_p = model.predict(inputs)
        assert np.array_equal(one["global_attention"].view(np.uint32), ga_p.view(np.uint32))
        if mode == "leave_one_out":
            assert np.array_equal(one["contribution"][amask][:, 0], np.repeat(raw["y"], np.diff(pk.mol_offset)) - raw["ablated"])
    s = SCANN.__new__(SCANN)
    s.model, s.mean, s.std = model, 1.5, 0.25
    raw, got = model.atom_contributions(inputs), s.atom_contributions(inputs)
    real = amask[..., None]
    assert np.array_equal(got["y"], raw["y"] * 0.25 + 1.5)
    assert np.array_equal(got["ablated"], np.where(real, raw["ablated"] * 0.25 + 1.5, 0), equal_nan=True)
    assert np.array_equal(got["contribution"], raw["contribution"] * 0.25, equal_nan=True)


def test_cli_writes_the_contributions(hip_lib, tmp_path):
    """predict_model.py --contributions: contributions_<target>.pickle, one unpadded de-normalised dict per structure; the other files'
    bytes are those of a run without the flag"""
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
    assert not os.path.exists(out / "contributions_homo.pickle")
    r = subprocess.run(cli + ["--contributions", "leave_one_out"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    got = pickle.load(open(out / "contributions_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    i = 0
    for b in range(len(scann.dataIter)):
        inputs, _ = scann.dataIter[b]
        ref = scann.atom_contributions(inputs)
        amask = np.asarray(inputs["atom_mask"]).reshape(ref["order"].shape) != 0
        for s in range(len(amask)):
            d = got[i]
            assert sorted(d) == ["ablated", "contribution", "global_attention", "order", "y"]
            assert d["y"] == float(ref["y"][s, 0]) and np.array_equal(d["ablated"], ref["ablated"][s][amask[s]])
            assert np.array_equal(d["contribution"], ref["contribution"][s][amask[s]])
            assert sorted(d["order"].tolist()) == list(range(int(amask[s].sum())))
            i += 1
    assert i == n == len(got)


def test_limit_on_atoms_per_structure(hip_lib):
    """a structure of SCANN_ABLATE_MAX_ATOMS atoms is computed (a few of its entries against the reference: all of them would be
    n^3 d on the CPU); one atom more is refused with SCANN_ERR_UNSUPPORTED and a message naming the limit"""
    import size_batches
    from scann import _hip

    lim = _hip.ABLATE_MAX_ATOMS
    cfg, w, inputs, pk, model = setup(kind="qm9", L=2, data=size_batches.giant_data(lim))
    entries = {0: None, 1: [0, 1, 31, 32, 500, lim - 2, lim - 1], 2: None}
    for mode in MODES:
        got = run(model, pk, mode)
        ablate_ref.check_order(got["order"], got["ga"], pk.mol_offset)
        assert np.isfinite(got["ablated"][pk.mol_offset[1]:pk.mol_offset[2]]).sum() >= lim - 2
        ent = {s: (list(range(pk.mol_offset[s + 1] - pk.mol_offset[s])) if e is None else e) for s, e in entries.items()}
        with np.errstate(all="ignore"):
            refs = []
            for dt in (np.float64, np.float32):
                z, mol = ablate_ref.after_lc(cfg, w, inputs, dt)
                refs.append(ablate_ref.ablate(cfg, w, z, mol, mode, got["order"], dt, entries=ent)[0])
        sel = np.concatenate([pk.mol_offset[s] + np.asarray(e) for s, e in ent.items()])
        ablate_ref.check_ablated(got["ablated"][sel], refs[0][sel], refs[1][sel], "giant %d %s" % (lim, mode))
    cfg, w, inputs, pk, model = setup(kind="qm9", L=2, data=size_batches.giant_data(lim + 1))
    rb = model.engine.upload(pk)
    with pytest.raises(_hip.ScannHipError) as e:
        model.engine.ablate_pooling(rb, "deletion")
    assert e.value.code == -2 and str(lim) in str(e.value)
    rb.free()


def test_mp2018_b128_leave_one_out(hip_lib):
    """about 3.2 k atoms in 128 MP2018-shaped structures: `ablated` within 1e-4 of the fp32 reference"""
    import size_batches

    cfg, w, inputs, pk, model = setup(kind="mp2018", data=size_batches.mp2018_b128_data())
    got = run(model, pk, "leave_one_out")
    with np.errstate(all="ignore"):
        z, mol = ablate_ref.after_lc(cfg, w, inputs, np.float32)
        ref, _ = ablate_ref.ablate(cfg, w, z, mol, "leave_one_out", got["order"], np.float32)
    assert np.array_equal(~np.isfinite(got["ablated"]), ~np.isfinite(ref))
    fin = np.isfinite(ref)
    e = rel_err(got["ablated"][fin], ref[fin])
    print("mp2018_b128 leave-one-out: %d atoms, rel_err against the fp32 reference %.3e" % (pk.n_atom, e))
    assert e <= 1e-4


if __name__ == "__main__":
    case, out = sys.argv[1], sys.argv[2]
    _, _, _, pk_, model_ = setup(**CASES[case])
    res = {}
    for mode_ in MODES:
        for k_, v_ in run(model_, pk_, mode_).items():
            res[mode_ + "_" + k_] = v_
    np.savez(out, **res)

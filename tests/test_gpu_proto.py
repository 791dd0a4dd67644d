"""GPU tests of the prototypes and criticisms of a latent index (scann_index_prototypes / scann_index_criticisms through
Engine.index_prototypes, index_criticisms; LatentIndex.prototypes, LatentIndex.mmd, HipModel.prototypes / nearest_prototype).  Every
comparison of a device result with a twin is an equality of integers.

1. The kernels == the twins scann_prototypes_host / scann_criticisms_host in positions, scores, b_at_pick, A, B, ids, atoms and tails:
   N either side of the 256-row tile, one and many workgroups, more than one range of the self-join, dim either side of the 32-column
   slab and no multiple of 4, the smallest and the largest widths, two storage chunks; m = 1, a few, beyond N; planted duplicates, a
   non-finite row; criticisms in both witness modes.  2. One add or many; after unrelated indices were created and freed.  3. End to
   end on the qm9 and mp2018 fixtures at both levels.  4. Non-interference on an inference handle and a training twin.  5. Errors.  6. The CLI."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import proto_ref  # noqa: E402
from analysis_checks import _bits, make_index, random_rows, same_arrays, scan_edge_rows, setup, training_twin, untouched  # noqa: E402
from test_gpu_peaks import gamma_for  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def names_for(n):
    return np.arange(n, dtype=np.int64) * 3 + 5, (np.arange(n) % 7).astype(np.int32)


def same_prototypes(got, want, ids, atoms, label):
    """the device's dict against the twin's: every integer, the names of the picks, the tails"""
    c = int(want["count"])
    assert int(got["count"]) == c, label + ": count"
    for key in ("position", "score", "b_at_pick", "A", "B"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), label + ": " + key
    pos = want["position"][:c]
    assert np.array_equal(got["id"][:c], ids[pos]) and np.array_equal(got["atom"][:c], atoms[pos]), label + ": names"
    assert (got["position"][c:] == -1).all() and (got["id"][c:] == -1).all() and (got["atom"][c:] == -1).all(), label + ": tails"
    assert (got["score"][c:] == 0).all() and (got["b_at_pick"][c:] == 0).all(), label + ": tails"


def same_criticisms(got, want, ids, atoms, label):
    c = int(want["count"])
    assert int(got["count"]) == c, label + ": count"
    assert np.array_equal(got["position"], want["position"]) and np.array_equal(got["score"], want["score"]), label
    pos = want["position"][:c]
    assert np.array_equal(got["id"][:c], ids[pos]) and np.array_equal(got["atom"][:c], atoms[pos]), label + ": names"
    assert (got["position"][c:] == -1).all() and (got["id"][c:] == -1).all() and (got["score"][c:] == 0).all(), label + ": tails"


def check_pool(eng, rows, ms, gamma, label, crit=0, ix=None):
    """the device calls on an index of ``rows`` against the twins, for every m of ``ms``; returns the last device result"""
    from scann import _hip
    from scann.models import latent_index as li

    ids, atoms = names_for(len(rows))
    own = ix is None
    if own:
        ix = make_index(eng, rows, ids, atoms)
    try:
        for m in ms:
            got, want = eng.index_prototypes(ix, m, gamma), _hip.prototypes_host(rows, m, gamma)
            same_prototypes(got, want, ids, atoms, "%s m %d" % (label, m))
            c = int(got["count"])
            n = int((got["A"] >= 0).sum())
            assert c == min(m, n)
            if c:  # the first pick is the densest row, ties to the lowest position
                assert got["position"][0] == int(np.argmax(got["A"])) and got["score"][0] == got["A"].max() and got["b_at_pick"][0] == 0
            for wit in ("under", "both") if crit and c else ():
                _, _, weight = li.prototypes_weights(got["A"], got["B"], c, wit)
                ex = got["position"][:c]
                gc, wc = eng.index_criticisms(ix, weight, ex, crit, gamma), _hip.criticisms_host(rows, weight, ex, crit, gamma)
                same_criticisms(gc, wc, ids, atoms, "%s m %d criticisms %s" % (label, m, wit))
                assert not set(gc["position"][:gc["count"]].tolist()) & set(ex.tolist())
                print("%s m %d %s: %d criticisms, scores %s" % (label, m, wit, gc["count"], gc["score"][:3]))
    finally:
        if own:
            ix.free()
    print("%s: gamma %.3g, %d eligible, picks %s, scores %s" % (label, gamma, n, got["position"][:4], got["score"][:3]))
    return got


# ---- 1. the kernels against the twins ----

@pytest.mark.parametrize("N,dim,crit", [(1, 128, 0), (100, 130, 6), (255, 1, 0), (256, 3, 0), (257, 130, 0), (1000, 128, 9), (5000, 130, 0),
                                        (20000, 128, 0), (600, 1024, 5)])
def test_kernels_equal_the_host_twins(engine, N, dim, crit):
    rows = random_rows(N, dim)
    if N == 257:
        rows[200, 129] = np.nan
        rows[13, 0] = np.inf
    ms = (1, 7, N + 3) if N <= 257 else (33 + N % 32,)
    got = check_pool(engine, rows, ms, gamma_for(rows), "N %d dim %d" % (N, dim), crit=crit)
    if N == 257:
        assert got["A"][200] == -1 and got["A"][13] == -1 and got["B"][200] == 0 and got["count"] == 255
        assert 200 not in got["position"] and 13 not in got["position"]
    if N >= 100 and N <= 257 and dim > 1:
        # random_rows' duplicates of row 3 share A and B throughout: they are picked in position order (every row is picked: m > N)
        dup = [3] + list(range(N // 2, N // 2 + 4))
        at = {int(p): s for s, p in enumerate(got["position"][:got["count"]])}
        assert [at[d] for d in dup] == sorted(at[d] for d in dup)
        assert len({int(got["A"][d]) for d in dup}) == 1 and len({int(got["B"][d]) for d in dup}) == 1


def test_criticisms_at_the_edges_of_the_eligibility_scan(engine):
    """every row weighs 1, so that the scan alone decides which rows live; with c beyond N the picks go on until no live row has a score
    left, and none of them is a row with a non-finite component"""
    from scann import _hip

    for label, rows in scan_edge_rows():
        N = len(rows)
        ok = np.isfinite(rows).all(axis=1)
        ids, atoms = names_for(N)
        weight = np.ones(N, np.int64)
        ix = make_index(engine, rows, ids, atoms)
        try:
            got = engine.index_criticisms(ix, weight, None, N + 2, 0.05)
        finally:
            ix.free()
        same_criticisms(got, _hip.criticisms_host(rows, weight, None, N + 2, 0.05), ids, atoms, label)
        assert got["count"] > 0 and ok[got["position"][:got["count"]]].all(), label


def test_duplicates_and_coincident_rows(engine):
    from scann import _hip
    import kcenter_ref

    ints = proto_ref.peaks_ref.small_integer_rows(300, 9, seed=2)
    ints[50:60] = ints[3]
    ints[77, 2] = np.nan
    g = check_pool(engine, ints, (12,), 0.02, "small integers", crit=4)
    r = proto_ref.prototypes(ints, 12, kcenter_ref.exact_dist2, _hip.rbf_weight, 0.02)
    assert g["position"].tolist() == r["position"] and g["score"].tolist() == r["score"] and g["b_at_pick"].tolist() == r["b_at_pick"]
    assert g["A"].tolist() == r["A"] and g["B"].tolist() == r["B"]
    proto_ref.certificate(ints[:100], engine_picks(engine, ints[:100], 6, 0.02), kcenter_ref.exact_dist2, _hip.rbf_weight, 0.02)
    same = np.tile(ints[:1], (300, 1))
    g = check_pool(engine, same, (5,), 0.5, "all coincident", crit=3)
    assert g["position"].tolist() == [0, 1, 2, 3, 4] and (g["A"] == 300 * 2 ** 30).all() and (g["B"] == 5 * 2 ** 30).all()
    assert g["score"].tolist() == [300 * 2 ** 30] * 5  # (s + 1) 300 2^30 - 300 s 2^30


def engine_picks(eng, rows, m, gamma):
    ix = make_index(eng, rows)
    try:
        r = eng.index_prototypes(ix, m, gamma)
        return r["position"][:r["count"]]
    finally:
        ix.free()


def test_an_empty_pool(engine):
    ix = engine.index_create(8)
    try:
        r = engine.index_prototypes(ix, 3, 0.5)
        assert r["count"] == 0 and (r["position"] == -1).all() and r["A"].shape == (0,)
        c = engine.index_criticisms(ix, np.zeros(0, np.int64), None, 2, 0.5)
        assert c["count"] == 0 and (c["position"] == -1).all()
    finally:
        ix.free()


def test_two_storage_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns"""
    rows = random_rows(17000, 1024)
    rows[16990] = rows[16383]  # duplicates on either side of the chunk boundary
    got = check_pool(engine, rows, (40,), gamma_for(rows, u=3.0), "17,000 x 1,024", crit=6)
    # every row on either side of the boundary took the picks' columns, and the two copies went through the call as one
    assert (got["B"][:16384] > 0).all() and (got["B"][16384:] > 0).all() and got["count"] == 40
    assert got["A"][16990] == got["A"][16383] and got["B"][16990] == got["B"][16383]


# ---- 2. invariance ----

def test_results_do_not_depend_on_how_the_pool_was_built(engine):
    from scann.models import latent_index as li

    dim, N, m = 130, 3000, 40
    rows = random_rows(N, dim, seed=9)
    gamma = gamma_for(rows)
    one = make_index(engine, rows)
    first = engine.index_prototypes(one, m, gamma)
    weight = li.prototypes_weights(first["A"], first["B"], m)[2]
    first_c = engine.index_criticisms(one, weight, first["position"], 8, gamma)
    junk = [make_index(engine, random_rows(n, d, seed=n)) for n, d in ((500, 64), (9000, 1024), (100, 130))]
    for j in junk[::2]:
        j.free()
    many = engine.index_create(dim)
    try:
        at = 0
        for step in [1, 63, 64, 65, 7, 1000, 3, 500, 255, 257]:
            engine.index_add(many, rows[at:at + step])
            at += step
        engine.index_add(many, rows[at:])
        same_arrays(engine.index_prototypes(many, m, gamma), first, "many adds")
        same_arrays(engine.index_criticisms(many, weight, first["position"], 8, gamma), first_c, "many adds, criticisms")
        same_arrays(engine.index_prototypes(one, m, gamma), first, "repeat")
    finally:
        junk[1].free()
        one.free()
        many.free()


# ---- 3. end to end ----

E2E = {"qm9": 40, "mp2018": 24}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_prototypes_of_a_model_are_the_twins_on_its_rows(hip_lib, kind, level, tmp_path):
    from scann.models import LatentPrototypes
    from scann.models import latent_index as li

    n = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n, seed=0)
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    rows, ids, atoms = index.rows()
    res, pr = model.prototypes(index, 6, criticisms=4)
    want, pr_w = li.prototypes_rows_host(rows, 6, criticisms=4, ids=ids, atoms=atoms, level=level)
    print("%s %s: %d rows, bandwidth %.4g, picks %s, mmd2 %s, criticisms %s, sizes %s" % (
        kind, level, len(rows), res["bandwidth"], res["position"], res["mmd2"], res["criticism_position"], res["size"]))
    assert sorted(res) == sorted(want) and res["bandwidth"] == want["bandwidth"] and res["gamma"] == want["gamma"]
    for key in ("position", "id", "atom", "score", "b_at_pick", "A", "B", "criticism_position", "criticism_id", "criticism_atom",
                "criticism_score", "nearest_prototype", "size"):
        assert np.array_equal(res[key], want[key]), key
    for key in ("mmd2", "witness", "criticism_witness"):
        assert np.array_equal(res[key].view(np.uint64), want[key].view(np.uint64)), key
    assert res["count"] == 6 and (res["mmd2"] >= 0).all() and res["size"].sum() == len(rows)  # (a further pick may raise the MMD of so few rows)
    assert np.array_equal(_bits(pr.rows), _bits(rows[res["position"]])) and np.array_equal(_bits(pr.rows), _bits(pr_w.rows))
    assert np.array_equal(pr.ids, ids[res["position"]]) and np.array_equal(pr.criticism_ids, res["criticism_id"]) and pr.level == level
    host, _ = index.prototypes(6, criticisms=4, route="host")
    assert np.array_equal(host["position"], res["position"]) and np.array_equal(host["criticism_position"], res["criticism_position"])
    both, _ = index.prototypes(6, criticisms=4, witness="both", bandwidth=res["bandwidth"])
    both_w, _ = li.prototypes_rows_host(rows, 6, criticisms=4, witness="both", bandwidth=res["bandwidth"])
    assert np.array_equal(both["criticism_position"], both_w["criticism_position"]) and np.array_equal(both["position"], res["position"])
    # a prediction explained by its nearest prototype: nearest(k = 1) on the prototype rows
    pr.save(str(tmp_path / "pr.npz"))
    back = LatentPrototypes.load(model, str(tmp_path / "pr.npz"))
    near = model.nearest_prototype(data, back)
    ref = model.nearest(data, back.index_on(model), k=1)
    assert np.array_equal(near["prototype_id"], ref["neighbor_id"][..., 0]) and np.array_equal(_bits(near["distance"]), _bits(ref["distance"][..., 0]))
    assert np.array_equal(_bits(near["predict_property"]), _bits(ref["predict_property"]))
    if level == "structure":  # the data are the index's own rows: the labelling pass names the same prototype, a prototype names itself
        assert np.array_equal(near["prototype"], res["nearest_prototype"])
        assert np.array_equal(near["prototype"][res["position"]], np.arange(6)) and (near["distance"][res["position"]] == 0).all()
    # the same estimator between two indices: an index against itself is at 0, against a shifted copy above it
    shifted = li.LatentIndex(model, level).add_rows(rows + np.float32(0.5) * res["bandwidth"])
    zero, shift = index.mmd(index, res["bandwidth"]), index.mmd(shifted, res["bandwidth"], chunk=17)
    assert zero["mmd2"] == 0.0 and zero["numerator"] == 0 and shift["mmd2"] > 0 and shift["witness"].shape == (len(rows),)
    assert shift["numerator"] == proto_ref_numerator(rows, shifted.rows()[0], res["gamma"], shift["denominator"])
    shifted.free()
    back.free()
    index.free()


def proto_ref_numerator(a, b, gamma, den):
    from scann import _hip

    v = proto_ref.mmd_two(a, b, _hip.knn_dist2_matrix, _hip.rbf_weight, gamma)
    assert den % v.denominator == 0
    return v.numerator * (den // v.denominator)


# ---- 4. state ----

def test_nothing_else_changes(hip_lib):
    from scann.models import latent_index as li

    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool, rows = u.eng, u.pool, u.rows[0]
        gamma = gamma_for(rows)
        first = eng.index_prototypes(pool, 9, gamma)
        weight = li.prototypes_weights(first["A"], first["B"], 9)[2]
        c_first = eng.index_criticisms(pool, weight, first["position"], 5, gamma)

        def same(r):
            same_arrays(r[0], first, "repeat")
            same_arrays(r[1], c_first, "repeat, criticisms")

        u.repeat(lambda: (eng.index_prototypes(pool, 9, gamma), eng.index_criticisms(pool, weight, first["position"], 5, gamma)), same, 5, 16 << 20)


def test_training_handle(hip_lib):
    from scann import _hip
    from scann.models import latent_index as li

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows = random_rows(900, 128, seed=8)
    gamma = gamma_for(rows)
    ids, atoms = names_for(len(rows))

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, rows, ids, atoms)
        got = eng.index_prototypes(ix, 20, gamma)
        same_prototypes(got, _hip.prototypes_host(rows, 20, gamma), ids, atoms, "training handle")
        weight = li.prototypes_weights(got["A"], got["B"], 20)[2]
        same_criticisms(eng.index_criticisms(ix, weight, got["position"], 6, gamma), _hip.criticisms_host(rows, weight, got["position"], 6, gamma),
                        ids, atoms, "training handle, criticisms")
        ix.free()

    training_twin(cfg, w, pk, calls)


# ---- 5. errors ----

def test_errors_name_what_is_wrong(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows = random_rows(5, 4, seed=0)
    pool, foreign = make_index(eng, rows), make_index(other.engine, rows)
    P = _hip._ptr
    pos, score = np.full(3, 7, np.int32), np.full(3, 7, np.int64)
    weight, ex = np.ones(5, np.int64), np.zeros(1, np.int32)

    def message():
        return (eng.lib.scann_last_error(eng._h) or b"").decode()

    def proto(p=pool, m=3, gamma=0.5, ps=pos):
        return eng.lib.scann_index_prototypes(eng._h, None if p is None else p._h, m, gamma, P(ps), None, None, P(score), None, None, None)

    def crit(p=pool, wt=weight, e=ex, ne=1, c=3, gamma=0.5, ps=pos):
        return eng.lib.scann_index_criticisms(eng._h, None if p is None else p._h, P(wt), P(e), ne, c, gamma, P(ps), None, None, P(score))

    free0, _ = eng.device_memory()
    assert proto(p=None) == -1 and "scann_index_prototypes: null handle or pool" in message()
    assert proto(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert proto(m=0) == -1 and "m 0 is not >= 1" in message()
    assert proto(ps=None) == -1 and "pos is null" in message()
    assert proto(m=2 ** 30) == -1 and "5 rows" in message() and str(2 ** 30) in message() and "2^32" in message()
    assert crit(p=None) == -1 and "scann_index_criticisms: null handle or pool" in message()
    assert crit(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert crit(c=0) == -1 and "c 0 is not >= 1" in message()
    assert crit(wt=None) == -1 and "weight is null" in message()
    assert crit(e=None) == -1 and "exclude is null" in message()
    assert crit(ps=None) == -1 and "pos is null" in message()
    assert crit(wt=np.array([1, 1, 2 ** 31 + 1, 1, 1], np.int64)) == -1 and "weight[2]" in message()
    assert crit(wt=np.array([1, -1, 1, 1, 1], np.int64)) == -1 and "weight[1]" in message()
    assert crit(e=np.array([5], np.int32)) == -1 and "exclude[0] = 5" in message()
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert proto(gamma=g) == -1 and "gamma must be finite and > 0" in message(), g
        assert crit(gamma=g) == -1 and "gamma must be finite and > 0" in message(), g
    assert (pos == 7).all() and (score == 7).all() and free0 - eng.device_memory()[0] <= 8 << 20
    assert proto() == 3 and crit() == 3
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError, match="m must"):
        eng.index_prototypes(pool, 0, 0.5)
    with pytest.raises(ValueError, match="2\\^32"):
        eng.index_prototypes(pool, 2 ** 31, 0.5)
    with pytest.raises(ValueError, match="weight"):
        eng.index_criticisms(pool, np.ones(4, np.int64), None, 2, 0.5)
    with pytest.raises(ValueError, match="exclude"):
        eng.index_criticisms(pool, weight, [9], 2, 0.5)
    lat = model.build_index(data)
    for kw, word in ((dict(m=0), "m must"), (dict(m=2, criticisms=-1), "criticisms"), (dict(m=2, bandwidth=0.0), "bandwidth"),
                     (dict(m=2, neighbours=40), "neighbours"), (dict(m=2, witness="over"), "witness"), (dict(m=2, route="gpu"), "route"),
                     (dict(m=2, assign=1), "assign")):
        with pytest.raises(ValueError, match=word):
            lat.prototypes(**kw)
    with pytest.raises(ValueError):
        other.prototypes(lat, 2)  # another model's index
    with pytest.raises(ValueError, match="level"):
        model.prototypes(data, 2, level="bond")
    with pytest.raises(ValueError, match="prototypes"):
        model.nearest_prototype(data, "a set")
    with pytest.raises(ValueError, match="other must"):
        lat.mmd("an index", 1.0)
    for ix in (pool, foreign, lat):
        ix.free()


# ---- 6. the CLI ----

def test_cli_writes_and_loads_prototypes(hip_lib, tmp_path):
    """predict_model.py --prototypes writes prototypes_<target>.pickle and, with --prototypes-out, protos.npz, which --nearest-prototype
    loads back in the same run: nearest_prototype_<target>.pickle"""
    import pickle
    import subprocess
    import sys

    import yaml

    import scann_oracle as so
    from scann.models import SCANN, LatentPrototypes
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
    r = subprocess.run(cli + ["--prototypes", "5", "--criticisms", "3", "--prototypes-out", str(tmp_path / "protos.npz"), "--nearest-prototype",
                              str(tmp_path / "protos.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert {"prototypes_homo.pickle", "nearest_prototype_homo.pickle"} <= set(os.listdir(out))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    want, pr = scann.prototypes(pool, 5, criticisms=3)
    got = pickle.load(open(out / "prototypes_homo.pickle", "rb"))
    assert sorted(got) == sorted(want)
    for key in ("position", "id", "atom", "score", "b_at_pick", "A", "B", "criticism_position", "criticism_id", "nearest_prototype", "size", "mmd2"):
        assert np.array_equal(got[key], want[key]), key
    assert got["bandwidth"] == want["bandwidth"] and "bandwidth" in r.stdout and "prototype    0" in r.stdout and "criticism    0" in r.stdout
    saved = LatentPrototypes.load(scann.model, str(tmp_path / "protos.npz"))
    assert np.array_equal(_bits(saved.rows), _bits(pr.rows)) and np.array_equal(saved.ids, pr.ids) and np.array_equal(saved.atoms, pr.atoms)
    assert saved.bandwidth == pr.bandwidth and saved.m == 5 and len(saved.criticism_ids) == len(want["criticism_position"])
    per = pickle.load(open(out / "nearest_prototype_homo.pickle", "rb"))
    inputs, _ = data[0]
    first = scann.nearest_prototype(inputs, saved)
    amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
    assert len(per) == n and sorted(per[0]) == ["distance", "predict_property", "prototype", "prototype_atom", "prototype_id"]
    assert np.array_equal(per[0]["prototype"], first["prototype"][0][amask[0]]) and np.array_equal(_bits(per[0]["distance"]), _bits(first["distance"][0][amask[0]]))
    assert (per[0]["prototype"] >= 0).all() and per[0]["prototype"].max() < 5
    saved.free()
    pool.free()

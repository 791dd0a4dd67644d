"""GPU tests of the k-means clustering (scann_index_kmeans through Engine.index_kmeans, LatentIndex.cluster, HipModel.cluster /
assign).  Every comparison is exact: labels equal, dist2 and centres bit for bit.

1. Kernels against the host twin (scann_kmeans_host) on standard-normal rows with planted ties, seeded by the k-center picks: N below one
   tile of 128 rows, tile +- 1, more than one storage chunk; k ragged against the block of 64 centres, the k maximum; dim 1, the dim
   maximum, a dim that is no multiple of the slab of 32.  The twin reports n_iter >= 2 there, so the update really ran.
2. Independent of the twin: labels / dist2 == Engine.index_query (k = 1) against an index of the returned centres.
3. Small-integer rows against the NumPy-only restatement; the planted cases of tests/test_cluster_host.py on the device; init_pos == init;
   one add or many, and after unrelated indices were created and freed.
4. End to end on the qm9 and mp2018 fixtures at both levels: HipModel.cluster == the twin on index.rows(), the certificate of
   tests/kmeans_ref.py, assign on the same inputs reproduces the labels.
5. Non-interference: pool, weights, selected outputs, the batch's last y, a training handle's state; device memory.
6. Errors name what is wrong.  7. The CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import kmeans_ref
import scann_oracle as so
from analysis_checks import SUBNORMAL, _bits, make_index, scan_edge_rows, setup, training_twin, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def check_exact(eng, rows, init, max_iter, stop=0, label="", want=None, ix=None):
    """the device's clustering against the host twin's (or ``want``): everything, bit for bit"""
    from scann import _hip

    own = ix is None
    ix = make_index(eng, rows) if own else ix
    try:
        got = eng.index_kmeans(ix, init, max_iter, stop)
    finally:
        if own:
            ix.free()
    cen = rows[init] if np.asarray(init).dtype.kind in "iu" else init
    want = _hip.kmeans_host(rows, cen, max_iter, stop) if want is None else want
    print("%s: N %d, dim %d, k %d, max_iter %d, stop %d: n_iter %d (host %d), converged %s (host %s), %d labels differ, %d centre values differ" % (
        label, len(rows), rows.shape[1], len(cen), max_iter, stop, got["n_iter"], want["n_iter"], got["converged"], want["converged"],
        int((got["label"] != want["label"]).sum()), int((_bits(got["centre"]) != _bits(want["centre"])).sum())))
    kmeans_ref.same(got, want, label)
    return got


def random_case(N, dim, k):
    from scann import _hip

    rng = np.random.default_rng(N * 7 + dim * 3 + k)
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    if N >= 100:
        rows[N // 2:N // 2 + 4] = rows[3]  # ties
    pos = _hip.kcenter_host(rows, None, k)["position"]
    return rows, pos


# (N, dim, k, max_iter).  A tile is 128 rows, a centre block 64 centres, a slab 32 columns; a storage chunk holds 64 MiB of rows, i.e.
# 16,384 rows of 1,024 columns: 17,000 x 1,024 spans two chunks
RANDOM_CASES = [(1, 3, 1, 3), (100, 128, 7, 8), (255, 1, 2, 8), (256, 3, 9, 8), (257, 130, 5, 8), (1000, 3, 64, 8), (1000, 128, 65, 8),
                (5000, 130, 33, 8), (3000, 16, 256, 4), (2000, 8, 1024, 2), (600, 1024, 12, 3), (17000, 1024, 20, 3)]


@pytest.mark.parametrize("N,dim,k,max_iter", RANDOM_CASES, ids=["N%d_d%d_k%d" % c[:3] for c in RANDOM_CASES])
def test_kernels_exact_on_random_rows(engine, N, dim, k, max_iter):
    from scann import _hip

    rows, pos = random_case(N, dim, k)
    want = _hip.kmeans_host(rows, rows[pos], max_iter)
    if N > 1:
        assert want["n_iter"] >= 2, want["n_iter"]  # the update really ran
    ix = make_index(engine, rows)
    try:
        got = check_exact(engine, rows, rows[pos], max_iter, want=want, ix=ix, label="random")
        # independent of the twin: the k = 1 query of the same rows against an index of the returned centres
        cix = make_index(engine, got["centre"])
        try:
            q = engine.index_query(cix, rows, 1)
        finally:
            cix.free()
        assert np.array_equal(q["position"][:, 0], got["label"])
        assert np.array_equal(_bits(q["dist2"][:, 0]), _bits(got["dist2"]))
        # the initial centres by position, copied on the device: the same run
        check_exact(engine, rows, pos, max_iter, want=want, ix=ix, label="random, init_pos")
        # max_iter = 0: a pure assignment to the given centres
        zero = check_exact(engine, rows, rows[pos], 0, ix=ix, label="random, max_iter 0")
        assert zero["n_iter"] == 0 and np.array_equal(_bits(zero["centre"]), _bits(rows[pos]))
    finally:
        ix.free()


def test_kernels_exact_on_small_integers(engine):
    """many exact ties, and a reference that needs nothing of the library: the chain restated in NumPy alone"""
    rng = np.random.default_rng(4)
    for N, dim, k in ((3000, 3, 40), (700, 33, 5)):
        rows = rng.integers(-4, 5, (N, dim)).astype(np.float32)
        init = rows[rng.choice(N, k, replace=False)]
        want = kmeans_ref.kmeans(rows, init, 6, 0, kmeans_ref.fma_dist2)
        got = check_exact(engine, rows, init, 6, label="integers")
        kmeans_ref.same(got, want, "integers against NumPy")
        kmeans_ref.certificate(rows, got, kmeans_ref.fma_dist2)


def test_planted_cases_on_the_device(engine):
    from test_cluster_host import planted_cases

    for name, rows, init, max_iter, stop, check in planted_cases():
        got = check_exact(engine, rows, init, max_iter, stop, label=name)
        check(got)
    # an empty pool returns 0 with the centres as given
    init = np.float32([[1, 2, 3], [4, 5, 6]])
    got = check_exact(engine, np.zeros((0, 3), np.float32), init, 5, label="empty pool")
    assert got["n_iter"] == 0 and got["converged"] and np.array_equal(got["centre"], init) and not got["size"].any()
    # a wide pool with non-finite values in a late column and in the padding's neighbour (dim 130: stride 132)
    rng = np.random.default_rng(12)
    wide = (rng.standard_normal((700, 130)) * 2).astype(np.float32)
    wide[13, 129] = np.nan
    wide[300, 128] = np.inf
    wide[699, 0] = -np.inf
    got = check_exact(engine, wide, wide[[1, 50, 400]], 5, label="planted, wide")
    assert np.all(got["label"][[13, 300, 699]] == -1) and np.all(np.isposinf(got["dist2"][[13, 300, 699]])) and got["size"].sum() == 697


def test_edges_of_the_eligibility_scan(engine):
    """labels and dist2 say which rows the scan found eligible; the centres of the subnormal column carry frexp's exponent of its maximum"""
    for label, rows in scan_edge_rows():
        ok = np.isfinite(rows).all(axis=1)
        got = check_exact(engine, rows, rows[ok][:2], 3, label=label)
        assert np.array_equal(got["label"] >= 0, ok) and np.array_equal(np.isposinf(got["dist2"]), ~ok), label
        if rows.shape[1] >= 5:
            assert got["centre"][:, 1].all() and (np.abs(got["centre"][:, 1]) < 400 * SUBNORMAL).all(), label


def test_invariance_of_how_the_index_was_built(engine):
    rng = np.random.default_rng(9)
    dim, N, k = 130, 3000, 21
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    rows[1500:1510] = rows[3]
    init = rows[rng.choice(N, k, replace=False)]
    one, many = engine.index_create(dim), engine.index_create(dim)
    try:
        engine.index_add(one, rows)
        at = 0
        for step in [1, 63, 64, 65, 7, 1000, 3, 500, 255, 257]:
            engine.index_add(many, rows[at:at + step])
            at += step
        while at < N:
            engine.index_add(many, rows[at:at + 311])
            at += 311
        a = check_exact(engine, rows, init, 6, ix=one, label="one add")
        # unrelated indices come and go in between (the workspace and the chunks come from the same block cache)
        for d in (64, 130, 7):
            tmp = make_index(engine, rng.standard_normal((900, d)).astype(np.float32))
            engine.index_kmeans(tmp, np.arange(5), 3)
            tmp.free()
        for ix in (many, one):
            check_exact(engine, rows, init, 6, ix=ix, want=a, label="many adds")
        # a shorter run that did not converge is where the longer one was then
        b = engine.index_kmeans(one, init, 2)
        assert b["n_iter"] == 2 and a["n_iter"] > 2
    finally:
        one.free()
        many.free()


# ---- end to end ----

E2E = {"qm9": (64, 6), "mp2018": (24, 4)}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_cluster_is_the_host_clustering_of_the_models_rows(hip_lib, kind, level):
    from scann import _hip
    from scann.models import LatentClustering

    n, k = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n, seed=0)
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    rows, ids, atoms = index.rows()
    got, clustering = model.cluster(index, k, max_iter=8)
    pos = _hip.kcenter_host(rows, None, k)["position"]
    want = _hip.kmeans_host(rows, rows[pos], 8)
    raw = model.engine.index_kmeans(index._ix, pos, 8)
    kmeans_ref.same(raw, want, "%s %s" % (kind, level))
    kmeans_ref.certificate(rows, raw, _hip.knn_dist2_matrix)
    assert np.array_equal(got["label"], want["label"]) and np.array_equal(_bits(got["distance"]), _bits(np.sqrt(want["dist2"])))
    assert np.array_equal(_bits(got["centre"]), _bits(want["centre"])) and np.array_equal(got["size"], want["size"])
    assert got["n_iter"] == want["n_iter"] and got["converged"] == want["converged"]
    assert got["inertia"] == float(want["dist2"][want["label"] >= 0].astype(np.float64).sum())
    for c in range(k):  # the medoid: the member first under (dist2, position)
        member = np.nonzero(want["label"] == c)[0]
        m = member[np.lexsort((member, want["dist2"][member]))][0] if len(member) else -1
        assert got["medoid_position"][c] == m
        assert got["medoid_id"][c] == (ids[m] if m >= 0 else -1) and got["medoid_atom"][c] == (atoms[m] if m >= 0 else -1)
    assert isinstance(clustering, LatentClustering) and clustering.level == level and np.array_equal(_bits(clustering.centres), _bits(want["centre"]))
    # assign on the same inputs reproduces the labels and the distances
    a = model.assign(data, clustering, batch_size=16)
    if level == "structure":
        assert a["cluster"].dtype == np.int32 and np.array_equal(a["cluster"], want["label"])
        assert np.array_equal(_bits(a["distance"]), _bits(got["distance"]))
    else:
        assert np.array_equal(a["cluster"], _hip.repad_atoms(want["label"], data["atom_mask"], -1))
        assert np.array_equal(_bits(a["distance"]), _bits(_hip.repad_atoms(got["distance"], data["atom_mask"], 0)))
    y, _ = model.predict(data)
    assert np.array_equal(_bits(a["predict_property"]), _bits(y))
    # data instead of an index: indexed for the call and freed; the same clustering
    direct, c2 = model.cluster(data, k, level=level, max_iter=8, batch_size=16)
    assert np.array_equal(direct["label"], got["label"]) and np.array_equal(_bits(direct["centre"]), _bits(got["centre"]))
    assert np.array_equal(direct["medoid_id"] * 2 + 1, got["medoid_id"])  # (ids 0 .. n-1 there; -1 stays -1)
    clustering.free()
    c2.free()
    index.free()


# ---- state, errors ----

def test_nothing_else_changes(hip_lib):
    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool = u.eng, u.pool
        first = eng.index_kmeans(pool, np.arange(7) * 3, 6)

        def call():
            r = eng.index_kmeans(pool, np.arange(7) * 3, 6)
            eng.index_kmeans(pool, u.rows[0][:3], 0)
            return r

        u.repeat(call, lambda r: kmeans_ref.same(r, first, "repeat"), 10, 16 << 20)


def test_training_handle(hip_lib):
    """after two training steps a clustering on the training handle equals the host twin's, and weights, gradients and the following
    (deterministic) step are those of a twin that never made the call"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows, pos = random_case(900, 128, 11)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        check_exact(eng, rows, pos, 5, label="training handle")

    training_twin(cfg, w, pk, calls)


def test_generic_width_handle(hip_lib):
    """a handle of widths other than 128 / 8: rows of 32 and 96 columns"""
    from scann import _hip

    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=32)
    for level in ("structure", "atom"):
        ix = model.build_index(data, level=level, batch_size=4)
        rows = ix.rows()[0]
        got = ix.cluster(3, max_iter=6)
        want = _hip.kmeans_host(rows, rows[_hip.kcenter_host(rows, None, 3)["position"]], 6)
        assert np.array_equal(got["label"], want["label"]) and np.array_equal(_bits(got["centre"]), _bits(want["centre"]))
        assert got["n_iter"] == want["n_iter"]
        ix.free()


def test_errors_name_what_is_wrong(hip_lib):
    import ctypes as C

    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows = np.arange(12, dtype=np.float32).reshape(3, 4)
    rows_bad = rows.copy()
    rows_bad[1, 2] = np.nan
    pool, dirty, foreign = make_index(eng, rows), make_index(eng, rows_bad), make_index(other.engine, rows)
    out = {"label": np.full(3, 7, np.int32), "centre": np.full((2, 4), 7, np.float32)}
    init = rows[:2].copy()
    bad_init = init.copy()
    bad_init[1, 3] = np.inf
    P = _hip._ptr

    def call(p=pool, k=2, init=init, pos=None, max_iter=3, stop=0, labels=out["label"], centres=out["centre"], handle=eng):
        return eng.lib.scann_index_kmeans(handle._h, None if p is None else p._h, k, P(init), P(pos), max_iter, stop, P(labels), None, P(centres),
                                          None, None)

    def message(e=eng):
        return (eng.lib.scann_last_error(e._h) or b"").decode()

    free0, _ = eng.device_memory()
    assert call(p=None) == -1 and "null" in message()
    assert call(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert call(handle=other.engine) == -1 and "another handle" in message(other.engine)
    assert call(k=0) == -1 and "k 0" in message()
    assert call(k=1025) == -1 and "k 1025" in message() and "1024" in message()
    assert call(init=None) == -1 and "init" in message() and "neither" in message()
    assert call(pos=np.int32([0, 1])) == -1 and "init_pos" in message() and "both" in message()
    assert call(init=bad_init) == -1 and "non-finite" in message() and "centre 1" in message()
    assert call(init=None, pos=np.int32([0, 3])) == -1 and "init_pos[1] = 3" in message()
    assert call(init=None, pos=np.int32([-1, 2])) == -1 and "init_pos[0] = -1" in message()
    assert call(max_iter=-1) == -1 and "max_iter -1" in message()
    assert call(stop=-2) == -1 and "stop_changed -2" in message()
    assert call(labels=None) == -1 and "labels is null" in message()
    assert call(centres=None) == -1 and "centres is null" in message()
    assert call(p=dirty, init=None, pos=np.int32([0, 1])) == -1 and "init_pos[1] = 1" in message() and "non-finite" in message()
    # nothing was written, nothing stays allocated
    assert np.all(out["label"] == 7) and np.all(out["centre"] == 7)
    assert free0 - eng.device_memory()[0] <= 1 << 20
    assert call(init=None, pos=np.int32([0, 2])) >= 0 and out["label"].tolist() == [0, 0, 1]  # (row 1 lies between them: the tie goes to centre 0)
    assert call(p=dirty, init=None, pos=np.int32([0, 2])) >= 0 and out["label"][1] == -1
    # the Python layers: ValueError before any device call
    for kw in (dict(init=np.arange(2), max_iter=-1), dict(init=np.arange(2), stop_changed=-1), dict(init=np.int64([0, 9])), dict(init=bad_init),
               dict(init=np.zeros((2, 3), np.float32)), dict(init=np.zeros((0, 4), np.float32)), dict(init=np.arange(2), max_iter=2.5)):
        with pytest.raises(ValueError):
            eng.index_kmeans(pool, **kw)
    lat = model.build_index(data)
    for kw in (dict(k=0), dict(k=1025), dict(k=2, max_iter=-1), dict(k=2, stop_changed=-1), dict(k=2, init="random"), dict(k=2, init=[0, 1, 2]),
               dict(k=2, init=[0, 99]), dict(k=2, init=np.zeros((2, 5), np.float32)), dict(k=5)):  # (5 clusters of 4 rows)
        with pytest.raises(ValueError):
            lat.cluster(**kw)
    with pytest.raises(ValueError):
        other.cluster(lat, 2)
    with pytest.raises(ValueError):
        model.cluster(data, 2, level="bond")
    with pytest.raises(ValueError):
        model.assign(data, "a clustering")
    for ix in (pool, dirty, foreign, lat):
        ix.free()
    assert C.sizeof(C.c_int64) == 8


def test_cli_writes_the_clustering(hip_lib, tmp_path):
    """predict_model.py --cluster 3: clusters_<target>.pickle and, with --cluster-out, the centres; the other files' bytes are those of a
    run without the flag"""
    import yaml

    from scann.models import SCANN, LatentClustering
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
    listed = set(os.listdir(out))
    r = subprocess.run(cli + ["--cluster", "3", "--cluster-iter", "6", "--cluster-out", str(tmp_path / "kinds.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"clusters_homo.pickle"}
    got = pickle.load(open(out / "clusters_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    want, clustering = scann.cluster(pool, 3, max_iter=6)
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    assert got["size"].sum() == len(pool) and "n_iter %d" % want["n_iter"] in r.stdout and "medoid id %d atom %d" % (
        want["medoid_id"][0], want["medoid_atom"][0]) in r.stdout
    saved = LatentClustering.load(scann.model, str(tmp_path / "kinds.npz"))
    assert saved.level == "atom" and np.array_equal(_bits(saved.centres), _bits(want["centre"]))
    clustering.free()
    pool.free()

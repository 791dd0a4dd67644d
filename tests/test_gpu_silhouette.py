"""GPU tests of the silhouette of a labelled latent index (scann_index_silhouette through Engine.index_silhouette; LatentIndex.silhouette /
choose_k, HipModel.silhouette / choose_k, predict_model.py --cluster-sweep).  Every comparison of a device result with the host twin
scann_silhouette_host is an equality: counts, sums and other equal, a and b bit for bit.

1. The kernel == the twin: N either side of the 64-row tile and of the 128-query tile, dim either side of the 32-column slab and no
   multiple of 4; unlabelled rows, an empty cluster, a singleton, non-finite and coincident rows; cluster sizes 63 / 64 / 65 side by side;
   one cluster; 1,024 clusters over 1,500 rows.  2. Two storage chunks.  3. One add or many, qpos in any order.  4. The range error, and
   the next call.  5. Non-interference; a generic width; a training handle.  6. End to end on a small model; the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import scann_oracle as so  # noqa: E402
import silhouette_ref as sr  # noqa: E402
from analysis_checks import make_index, random_rows, setup, training_twin, untouched  # noqa: E402

pytestmark = pytest.mark.gpu
METRICS = ("euclidean", "sqeuclidean")


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def check_pool(eng, ix, rows, lab, n_clusters, metric, qpos=None, label="", shift=None):
    """the device call on an index of ``rows`` against the twin: every output; returns the device's dict"""
    from scann import _hip

    shift = sr.shift_for(rows, metric) if shift is None else shift
    got = eng.index_silhouette(ix, lab, n_clusters, qpos, metric, shift, table=True)
    sr.same(got, _hip.silhouette_host(rows, lab, n_clusters, qpos, metric, shift, table=True), label)
    plain = eng.index_silhouette(ix, lab, n_clusters, qpos, metric, shift)  # without the table: the same a, b, other
    assert "sums" not in plain
    for key in plain:
        assert plain[key].tobytes() == got[key].tobytes(), label + ": " + key + " without the table"
    return got


# ---- 1. the kernel against the twin ----

@pytest.mark.parametrize("dim", [3, 128, 130])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 129, 700])
def test_kernel_equals_the_host_twin(engine, N, dim):
    rows, lab = sr.pathological_case(N, dim)
    ix = make_index(engine, rows)
    try:
        for metric in METRICS:
            got = check_pool(engine, ix, rows, lab, 5, metric, label="N %d dim %d %s" % (N, dim, metric))
            cnt = sr.counting_rows(rows, lab)
            assert got["count"].sum() == cnt.sum() and got["count"][3] == 0 and (got["sums"][~cnt] == -1).all()
            if N >= 60:
                assert (got["sums"][cnt][:, :3] > 0).all() and np.isfinite(got["b"][cnt]).all() and got["a"][N - 1] == 0.0
                q = np.array([N - 1, 0, 10, 41, 41, 5, 62], np.int32)
                part = check_pool(engine, ix, rows, lab, 5, metric, q, "a qpos subset")
                assert np.array_equal(part["sums"], got["sums"][q]) and part["a"].tobytes() == got["a"][q].tobytes()
    finally:
        ix.free()


def test_cluster_sizes_around_the_tile(engine):
    """clusters of 63, 64, 65, 1 and 128 rows side by side, their rows interleaved by position: whole, nearly whole and barely begun
    padded tiles, and a cluster that ends exactly on a tile"""
    sizes = [63, 64, 65, 1, 128]
    rng = np.random.default_rng(3)
    lab = rng.permutation(np.repeat(np.arange(5), sizes)).astype(np.int32)
    rows = (rng.standard_normal((len(lab), 40)) + lab[:, None]).astype(np.float32)
    ix = make_index(engine, rows)
    try:
        for metric in METRICS:
            got = check_pool(engine, ix, rows, lab, 5, metric, label="63 / 64 / 65")
            assert got["count"].tolist() == sizes
        # the restated definition itself, at this size
        shift = sr.shift_for(rows, "euclidean")
        sr.same(engine.index_silhouette(ix, lab, 5, None, "euclidean", shift, table=True), sr.silhouette(rows, lab, 5, None, False, shift))
    finally:
        ix.free()


def test_one_cluster_and_a_thousand(engine):
    rows = random_rows(1500, 20, seed=5)
    ix = make_index(engine, rows)
    try:
        got = check_pool(engine, ix, rows, np.zeros(1500, np.int32), 1, "euclidean", label="C = 1")
        assert np.isnan(got["b"]).all() and (got["other"] == -1).all() and (got["a"] > 0).all()
        # 1,024 clusters over 1,500 rows: most clusters have one or two rows and most of every tile is padding
        lab = (np.random.default_rng(0).permutation(1500) % 1024).astype(np.int32)
        for metric in METRICS:
            got = check_pool(engine, ix, rows, lab, 1024, metric, label="C = 1024")
        assert got["count"].max() == 2 and got["count"].min() == 1 and (got["a"][lab >= 476] == 0).all() and (got["other"] >= 0).all()
        # a few clusters empty, the last ones among them
        got = check_pool(engine, ix, rows, np.where(lab % 7 == 0, -1, lab % 900).astype(np.int32), 1024, "euclidean", label="C = 1024, gaps")
        assert (got["count"][900:] == 0).all()
    finally:
        ix.free()


def test_more_queries_than_one_slice_of_the_table(engine):
    """the queries go in slices whose device table [slice][C] stays within 512 MiB: 65,536 queries at C = 1,024.  70,000 positions (with
    repeats) of a 700-row pool cross that switch; every one gets the row of the full answer"""
    from scann import _hip

    rows, _ = sr.pathological_case(700, 3)
    lab = (np.random.default_rng(6).permutation(700) * 3 % 1024).astype(np.int32)
    lab[::9] = -1
    shift = sr.shift_for(rows, "euclidean")
    q = np.random.default_rng(7).integers(0, 700, 70000).astype(np.int32)
    q[65535:65538] = [699, 0, 10]
    ix = make_index(engine, rows)
    try:
        full = check_pool(engine, ix, rows, lab, 1024, "euclidean", label="the pool itself")
        part = engine.index_silhouette(ix, lab, 1024, q, "euclidean", shift)
        twin = _hip.silhouette_host(rows, lab, 1024, q, "euclidean", shift)
        for key in ("a", "b", "other"):
            assert part[key].tobytes() == full[key][q].tobytes() == twin[key].tobytes(), key
        assert np.array_equal(part["count"], full["count"])
    finally:
        ix.free()


# ---- 2. two storage chunks ----

def test_two_storage_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns; the full self-join, and 300 positions on either side of the
    boundary"""
    from scann import _hip

    rows = random_rows(17000, 1024)
    lab = (np.random.default_rng(1).integers(0, 3, 17000)).astype(np.int32)
    lab[::50] = -1
    ix = make_index(engine, rows)
    try:
        mo = engine.index_moments(ix)
        shift = _hip.silhouette_shift(mo["col_exp"], np.diagonal(mo["cov"]), "euclidean")
        assert shift == sr.shift_for(rows, "euclidean")
        full = engine.index_silhouette(ix, lab, 3, None, "euclidean", shift, table=True)
        sr.same(full, _hip.silhouette_host(rows, lab, 3, None, "euclidean", shift, table=True), "17,000 x 1,024")
        q = np.random.default_rng(2).choice(17000, 300, replace=False).astype(np.int32)
        q[:3] = [16383, 16384, 16999]
        part = engine.index_silhouette(ix, lab, 3, q, "euclidean", shift, table=True)
        for key in ("a", "b", "other", "sums"):
            assert part[key].tobytes() == full[key][q].tobytes(), key
        assert (part["sums"][lab[q] >= 0] > 0).all()
    finally:
        ix.free()


# ---- 3. invariance ----

def test_results_do_not_depend_on_how_the_pool_was_built(engine):
    dim, N = 130, 3000
    rows = random_rows(N, dim, seed=9)
    lab = (np.random.default_rng(4).integers(-1, 6, N)).astype(np.int32)
    shift = sr.shift_for(rows, "euclidean")
    one = make_index(engine, rows)
    first = engine.index_silhouette(one, lab, 6, None, "euclidean", shift, table=True)
    # unrelated indices come and go: the block cache hands the next index other chunks
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
        again = engine.index_silhouette(many, lab, 6, None, "euclidean", shift, table=True)
        for key in first:
            assert again[key].tobytes() == first[key].tobytes(), key
        # the order of qpos is the order of the answer, nothing else
        q = np.random.default_rng(5).permutation(N)[:700].astype(np.int32)
        shuffled = engine.index_silhouette(many, lab, 6, q, "euclidean", shift, table=True)
        ordered = engine.index_silhouette(one, lab, 6, np.sort(q), "euclidean", shift, table=True)
        back = np.argsort(q, kind="stable")
        for key in ("a", "b", "other", "sums"):
            assert shuffled[key].tobytes() == first[key][q].tobytes() and ordered[key].tobytes() == shuffled[key][back].tobytes(), key
    finally:
        junk[1].free()
        one.free()
        many.free()


# ---- 4. the range error ----

@pytest.mark.parametrize("metric", METRICS)
def test_range_error_on_the_device_and_the_next_call(engine, metric):
    from scann import _hip

    a = np.float32(0.99)
    rows = np.array([[a] * 3, [-a] * 3] * 100, np.float32)   # rows that span the bound of their column ranges
    lab = (np.arange(200) // 2 % 2).astype(np.int32)
    shift = sr.shift_for(rows, metric)
    ix = make_index(engine, rows)
    try:
        first = check_pool(engine, ix, rows, lab, 2, metric, label="the chosen shift")
        with pytest.raises(_hip.ScannHipError, match="RANGE") as e:
            engine.index_silhouette(ix, lab, 2, None, metric, shift + 2)
        assert "scann_index_silhouette" in str(e.value) and "shift %d" % (shift + 2) in str(e.value)
        with pytest.raises(_hip.ScannHipError, match="RANGE"):
            _hip.silhouette_host(rows, lab, 2, None, metric, shift + 2)
        again = check_pool(engine, ix, rows, lab, 2, metric, label="after the refusal")
        for key in first:
            assert again[key].tobytes() == first[key].tobytes(), key
        # a row that does not count, however far, raises nothing
        far = rows.copy()
        far[7] = np.float32(3e19)
        ix2 = make_index(engine, far)
        try:
            lab2 = lab.copy()
            lab2[7] = -1
            check_pool(engine, ix2, far, lab2, 2, metric, label="a far row without a label", shift=shift)
            with pytest.raises(_hip.ScannHipError, match="RANGE"):
                engine.index_silhouette(ix2, lab, 2, None, metric, -126)
        finally:
            ix2.free()
    finally:
        ix.free()


def test_an_empty_pool_and_errors_name_what_is_wrong(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    empty = eng.index_create(8)
    r = eng.index_silhouette(empty, np.zeros(0, np.int32), 3)
    assert r["count"].tolist() == [0, 0, 0] and r["a"].shape == (0,)
    rows, lab = sr.pathological_case(65, 4)
    lab = lab.astype(np.int32)
    pool, foreign = make_index(eng, rows), make_index(other.engine, rows)
    P = _hip._ptr
    cnt, a, b, oth = np.full(5, 7, np.int64), np.full(65, 7.0), np.full(65, 7.0), np.full(65, 7, np.int32)
    q = np.array([1, 65], np.int32)
    bad_lab = np.where(np.arange(65) == 9, 5, lab).astype(np.int32)

    def message():
        return (eng.lib.scann_last_error(eng._h) or b"").decode()

    def call(p=pool, labels=lab, c=5, qpos=None, nq=0, shift=0, counts=cnt, a_=a, b_=b, other_=oth):
        return eng.lib.scann_index_silhouette(eng._h, None if p is None else p._h, P(labels), c, P(qpos), nq, 0, shift, P(counts), P(a_), P(b_),
                                              P(other_), None)

    free0, _ = eng.device_memory()
    assert call(p=None) == -1 and "scann_index_silhouette: null handle or pool" in message()
    assert call(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert call(labels=None) == -1 and "labels is null" in message()
    assert call(counts=None) == -1 and "counts is null" in message()
    assert call(a_=None) == -1 and "a is null" in message()
    assert call(b_=None) == -1 and "b is null" in message()
    assert call(other_=None) == -1 and "other is null" in message()
    for c in (0, 1025):
        assert call(c=c) == -1 and "C %d outside 1 .. 1024" % c in message()
    for s in (-127, 127):
        assert call(shift=s) == -1 and "shift %d outside -126 .. 126" % s in message()
    assert call(labels=bad_lab) == -1 and "labels[9] = 5 outside -1 .. 4" in message()
    assert call(qpos=q, nq=2) == -1 and "qpos[1] = 65 outside 0 .. 64" in message()
    assert call(qpos=q, nq=-1) == -1 and "nq -1 outside" in message()
    assert (cnt == 7).all() and (a == 7).all() and (oth == 7).all() and free0 - eng.device_memory()[0] <= 8 << 20
    assert call() == 0 and call(qpos=q, nq=1) == 0
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError, match="labels"):
        eng.index_silhouette(pool, lab[:-1], 5)
    with pytest.raises(ValueError, match="shift"):
        eng.index_silhouette(pool, lab, 5, None, "euclidean", 200)
    lat = model.build_index(data)
    for kw, word in ((dict(metric="l1"), "metric"), (dict(route="gpu"), "route"), (dict(sample=0), "sample"), (dict(sample=[len(lat)]), "sample"),
                     (dict(sample=len(lat) + 1), "only"), (dict(n_clusters=2000), "n_clusters")):
        with pytest.raises(ValueError, match=word):
            lat.silhouette(np.zeros(len(lat), np.int32), **kw)
    with pytest.raises(ValueError, match="at most 1024 clusters"):
        lat.silhouette(np.arange(len(lat)) + 1100)
    with pytest.raises(ValueError):
        other.silhouette(lat, np.zeros(len(lat), np.int32))  # another model's index
    with pytest.raises(ValueError, match="LatentIndex"):
        model.silhouette("an index", [0])
    with pytest.raises(ValueError, match="ks"):
        model.choose_k(data, (0, 2))
    with pytest.raises(ValueError, match="level"):
        model.choose_k(data, (2, 3), level="bond")
    for ix in (empty, pool, foreign, lat):
        ix.free()


# ---- 5. state ----

def test_nothing_else_changes(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool, rows = u.eng, u.pool, u.rows[0]
        lab = (np.arange(len(pool)) % 4 - (np.arange(len(pool)) % 9 == 0)).astype(np.int32)
        shift = sr.shift_for(rows, "euclidean")
        first = eng.index_silhouette(pool, lab, 4, None, "euclidean", shift, table=True)
        sr.same(first, _hip.silhouette_host(rows, lab, 4, None, "euclidean", shift, table=True), "the model's rows")

        def same(again):
            assert all(again[k].tobytes() == first[k].tobytes() for k in first)

        u.repeat(lambda: eng.index_silhouette(pool, lab, 4, None, "euclidean", shift, table=True), same, 4, 16 << 20)


def test_training_handle(hip_lib):
    """after two training steps the call on the training handle equals the twin, and weights, gradients and the following
    (deterministic) step are those of a twin handle that never made the call"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows, lab = sr.pathological_case(700, 128, seed=3)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, rows)
        check_pool(eng, ix, rows, lab, 5, "euclidean", label="training handle")
        ix.free()

    training_twin(cfg, w, pk, calls)


def same_table(got, want, label):
    for key in ("k", "score", "inertia", "calinski_harabasz", "davies_bouldin", "n_iter", "converged"):
        assert got[key].tobytes() == want[key].tobytes(), "%s: %s" % (label, key)
    assert got["best_k"] == want["best_k"] and all(np.array_equal(x, y) for x, y in zip(got["size"], want["size"])), label
    for part in ("best", "silhouette"):
        for key, v in want[part].items():
            g = got[part][key]
            assert (np.asarray(g).tobytes() == np.asarray(v).tobytes()) if isinstance(v, np.ndarray) else (g == v or (g != g and v != v)), \
                "%s: %s %s" % (label, part, key)


def test_generic_width_handle(hip_lib):
    """rows of 30 and 96 columns, the first no multiple of 4"""
    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    for level, ks in (("structure", (2, 3)), ("atom", (2, 5))):
        index = model.build_index(data, level=level)
        got = index.choose_k(ks)
        same_table(got, index.choose_k(ks, route="host"), "generic " + level)
        index.free()


# ---- 6. end to end, the CLI ----

@pytest.mark.parametrize("level", ["structure", "atom"])
def test_choose_k_of_a_model_is_the_host_route_on_its_rows(hip_lib, level):
    from scann.models import latent_index as li

    n = 40
    cfg, w, data, model = setup(kind="qm9", n=n, seed=0)
    ids = np.arange(n) * 2 + 1
    index = model.build_index(data, level=level, batch_size=16, ids=ids)
    rows, rid, atoms = index.rows()
    ks = (2, 3, 5, 8)
    table, clustering = model.choose_k(data, ks, level=level, batch_size=16, ids=ids)
    print("%s: %d rows, k %s score %s best %d" % (level, len(rows), table["k"], np.round(table["score"], 4), table["best_k"]))
    same_table(table, index.choose_k(ks, route="host"), level + ": the index's host route")
    same_table(table, li.choose_k_rows_host(rows, ks, ids=rid, atoms=atoms), level + ": the rows alone")
    same_table(table, model.choose_k(index, ks)[0], level + ": an index instead of data")
    assert table["best_k"] == int(table["k"][np.nanargmax(table["score"])]) and clustering.k == table["best_k"]
    assert np.array_equal(clustering.centres, table["best"]["centre"]) and clustering.level == level
    # the silhouette alone: the device and the host route, all rows, a sample, the table
    lab = table["best"]["label"]
    for kw in (dict(), dict(sample=min(25, len(rows)), seed=3), dict(metric="sqeuclidean", table=True), dict(sample=np.array([5, 0, 7]))):
        dev, host = model.silhouette(index, lab, **kw), index.silhouette(lab, route="host", **kw)
        assert sorted(dev) == sorted(host)
        for key, v in host.items():
            assert (dev[key].tobytes() == v.tobytes()) if isinstance(v, np.ndarray) else (dev[key] == v or (v != v and dev[key] != dev[key])), key
    assert np.array_equal(model.silhouette(index, lab)["silhouette"], table["silhouette"]["silhouette"], equal_nan=True)
    clustering.free()
    index.free()


def test_cli_sweep_writes_a_clustering_that_assign_loads(hip_lib, tmp_path):
    """predict_model.py --cluster-sweep prints the table, pickles it and, with --cluster-out, saves the best clustering, which loads back;
    the other files' bytes are those of a run without the flag"""
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
    r = subprocess.run(cli + ["--cluster-sweep", "2,3,5", "--cluster-sample", "30", "--cluster-out", str(tmp_path / "best.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"cluster_sweep_homo.pickle"}
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    want, clustering = scann.choose_k(pool, (2, 3, 5), sample=30)
    got = pickle.load(open(out / "cluster_sweep_homo.pickle", "rb"))
    same_table(got, want, "the pickled table")
    assert "best k %d" % want["best_k"] in r.stdout and "silhouette" in r.stdout and "Davies-Bouldin" in r.stdout
    saved = LatentClustering.load(scann.model, str(tmp_path / "best.npz"))
    assert np.array_equal(saved.centres, clustering.centres) and saved.k == want["best_k"] and saved.level == "atom"
    inputs, _ = data[0]
    a, b = scann.assign(inputs, saved), scann.assign(inputs, clustering)
    assert np.array_equal(a["cluster"], b["cluster"]) and (a["cluster"].max() < want["best_k"])
    for x in (saved, clustering, pool):
        x.free()

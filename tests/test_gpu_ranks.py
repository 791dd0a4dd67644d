"""GPU tests of the exact neighbour ranks of a latent index (scann_index_ranks through Engine.index_ranks; LatentIndex.map_quality /
choose_perplexity, HipModel.map_quality / choose_perplexity, predict_model.py --map-quality / --embed-sweep).  Every comparison of a
device result with the host twin scann_ranks_host is an equality of bytes.

1. The kernel == the twin: N either side of the 64-row and the 128-query tile, dim either side of the 32-column slab, no multiple of 4
   and the 2-column map case, m = 1, 31, 32, on the pathological pool.  2. Ties beyond the probe count.  3. Many ranges per query; the
   permutation.  4. Two storage chunks; one add or many; qpos in any order; more queries than one slice.  5. The search's places have
   their ranks.  6. Non-interference; a generic width; a training handle.  7. End to end on a small model; the CLI.  8. Bad arguments."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import rank_ref as rr  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import make_index, random_rows, setup, training_twin, untouched  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def check_pool(eng, ix, rows, probe, qpos=None, label=""):
    """the device call on an index of ``rows`` against the twin: both outputs; returns the device's dict"""
    from scann import _hip

    got = eng.index_ranks(ix, probe, qpos, dist2=True)
    rr.same(got, _hip.ranks_host(rows, probe, qpos, dist2=True), label)
    plain = eng.index_ranks(ix, probe, qpos)                                     # without dist2: the same ranks
    assert "dist2" not in plain and plain["rank"].tobytes() == got["rank"].tobytes(), label + ": without dist2"
    return got


def same_quality(got, want, label):
    assert sorted(got) == sorted(want), label
    for key, v in want.items():
        assert np.asarray(got[key]).dtype == np.asarray(v).dtype and np.asarray(got[key]).tobytes() == np.asarray(v).tobytes(), "%s: %s" % (label, key)


# ---- 1. the kernel against the twin ----

@pytest.mark.parametrize("dim", [2, 3, 128, 130])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 129, 700])
def test_kernel_equals_the_host_twin(engine, N, dim):
    rows = rr.pathological_pool(N, dim)
    ix = make_index(engine, rows)
    try:
        for m in (1, 31, 32):
            got = check_pool(engine, ix, rows, rr.probe_lists(N, N, m, seed=m), label="N %d dim %d m %d" % (N, dim, m))
            assert N < 3 or (got["rank"] >= 0).any()
        if N >= 65:
            rr.same(got, rr.ranks(rows, rr.probe_lists(N, N, 32, seed=32)), "the restated definition itself")
            assert (got["rank"][10:12] == -1).all()                              # ineligible queries
            d = engine.index_ranks(ix, np.array([[62, 61]], np.int32), np.array([61], np.int32), dist2=True)
            assert np.isposinf(d["dist2"][0, 0]) and d["rank"][0, 0] >= 0 and d["rank"][0, 1] == -1  # +inf is an ordinary distance
    finally:
        ix.free()


# ---- 2. ties beyond the probe count ----

def test_ties_beyond_the_probe_count(engine):
    """40 coincident rows and 30 others: thresholds that are all equal in distance and differ in position only, seen from inside the
    run (distance 0) and from outside; the same position 32 times"""
    rows = rr.pathological_pool(70, 3)
    run = np.arange(20, 60, dtype=np.int32)
    q = np.array([20, 37, 59, 5, 69], np.int32)
    probe = np.stack([run[:32], run[8:], np.full(32, 44, np.int32), run[:32], run[::-1][:32]])
    ix = make_index(engine, rows)
    try:
        got = check_pool(engine, ix, rows, probe, q, "the coincident run")
        assert got["rank"][0].tolist() == [-1] + list(range(31))
        assert (got["rank"][2] == 24).all() and (got["dist2"][:3][got["rank"][:3] >= 0] == 0).all()
        assert np.array_equal(np.diff(got["rank"][3]), np.ones(31)) and np.array_equal(np.diff(got["rank"][4]), -np.ones(31))
        # every row of the pool probing the whole run, 32 at a time
        for part in (run[:32], run[8:]):
            check_pool(engine, ix, rows, np.tile(part, (70, 1)), label="all rows against the run")
    finally:
        ix.free()


# ---- 3. many ranges per query ----

def test_many_ranges_and_the_permutation(engine):
    """5,000 rows x 3: 79 ranges of one tile per query tile; a workgroup's counts meet in the table by atomics"""
    from scann import _hip
    from scann.models import latent_index as li

    N = 5000
    rows = random_rows(N, 3)
    rows[4000, 1] = np.nan
    n_el = N - 1
    ix = make_index(engine, rows)
    try:
        pos, _ = li.neighbour_graph_host(rows[:400])
        probe = np.random.default_rng(0).integers(-1, N, (N, 31)).astype(np.int32)
        probe[:400, :20] = pos[:, :20]                                           # near probes beside far ones
        check_pool(engine, ix, rows, probe, label="5,000 x 3")
        for i in (0, 3999, 4001, 2500, 2501, 2502, 4998, 4999):
            p = rr.all_others(N, i)
            q = np.full(len(p), i, np.int32)
            r = engine.index_ranks(ix, p, q)["rank"]
            assert r.tobytes() == _hip.ranks_host(rows, p, q)["rank"].tobytes()
            flat = r.reshape(-1)
            assert np.array_equal(np.sort(flat[flat >= 0]), np.arange(n_el - 1)) and (flat < 0).sum() == p.size - (n_el - 1), i
    finally:
        ix.free()


# ---- 4. storage and call shape ----

def test_two_storage_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns; the full self-join on the device, the twin on 200 positions on
    either side of the boundary"""
    from scann import _hip

    N = 17000
    rows = random_rows(N, 1024)
    probe = np.random.default_rng(1).integers(0, N, (N, 4)).astype(np.int32)
    probe[:, 0] = (np.arange(N) + 16384) % N                                     # across the boundary
    ix = make_index(engine, rows)
    try:
        full = engine.index_ranks(ix, probe, dist2=True)
        q = np.random.default_rng(2).choice(N, 200, replace=False).astype(np.int32)
        q[:3] = [16383, 16384, 16999]
        part = check_pool(engine, ix, rows, probe[q], q, "17,000 x 1,024")
        assert part["rank"].tobytes() == full["rank"][q].tobytes() and part["dist2"].tobytes() == full["dist2"][q].tobytes()
        assert (full["rank"] >= 0).sum() >= full["rank"].size - 32              # (a random probe may be the query itself)
    finally:
        ix.free()


def test_results_do_not_depend_on_how_the_pool_was_built(engine):
    dim, N = 130, 3000
    rows = random_rows(N, dim, seed=9)
    probe = rr.probe_lists(N, N, 31, seed=3)
    one = make_index(engine, rows)
    first = engine.index_ranks(one, probe, dist2=True)
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
        rr.same(engine.index_ranks(many, probe, dist2=True), first, "many add calls")
        # the order of qpos is the order of the answer, nothing else
        q = np.random.default_rng(5).permutation(N)[:700].astype(np.int32)
        shuffled = check_pool(engine, many, rows, probe[q], q, "a shuffled subset")
        ordered = engine.index_ranks(one, probe[np.sort(q)], np.sort(q), dist2=True)
        back = np.argsort(q, kind="stable")
        for key in ("rank", "dist2"):
            assert shuffled[key].tobytes() == first[key][q].tobytes() and ordered[key].tobytes() == shuffled[key][back].tobytes(), key
    finally:
        junk[1].free()
        one.free()
        many.free()


def test_more_queries_than_one_slice(engine):
    """the queries go in slices of 262,144: 262,300 positions (with repeats) of a 65-row pool cross that switch; every one gets the row of
    the full answer"""
    from scann import _hip

    rows = rr.pathological_pool(65, 2)
    n = _hip.RANKS_SLICE + 156
    q = np.random.default_rng(7).integers(0, 65, n).astype(np.int32)
    q[_hip.RANKS_SLICE - 1:_hip.RANKS_SLICE + 2] = [64, 0, 21]
    base = rr.probe_lists(65, 65, 2, seed=1)
    ix = make_index(engine, rows)
    try:
        full = check_pool(engine, ix, rows, base, label="the pool itself")
        part = engine.index_ranks(ix, base[q], q, dist2=True)
        twin = _hip.ranks_host(rows, base[q], q, dist2=True)
        for key in ("rank", "dist2"):
            assert part[key].tobytes() == full[key][q].tobytes() == twin[key].tobytes(), key
    finally:
        ix.free()


# ---- 5. agreement with the search ----

def test_the_search_places_have_their_ranks(engine):
    rows = np.random.default_rng(11).standard_normal((700, 128)).astype(np.float32)
    ix = make_index(engine, rows)
    try:
        r = engine.index_query(ix, rows, 32)
        assert (r["position"][:, 0] == np.arange(700)).all()                     # random rows: every row is its own nearest
        pos, d2 = r["position"][:, 1:], r["dist2"][:, 1:]
        got = check_pool(engine, ix, rows, pos, label="the search's places")
        assert (got["rank"] == np.arange(31)).all() and got["dist2"].tobytes() == d2.tobytes()
    finally:
        ix.free()


# ---- 6. state ----

def test_nothing_else_changes(hip_lib):
    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool = u.eng, u.pool
        probe = rr.probe_lists(len(pool), len(pool), 31, seed=9)
        first = check_pool(eng, pool, u.rows[0], probe, label="the model's rows")
        u.repeat(lambda: eng.index_ranks(pool, probe, dist2=True), lambda r: rr.same(r, first, "repeat"), 4, 16 << 20)


def test_training_handle(hip_lib):
    """after two training steps the call on the training handle equals the twin, and weights, gradients and the following
    (deterministic) step are those of a twin handle that never made the call"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows = rr.pathological_pool(700, 128, seed=3)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, rows)
        check_pool(eng, ix, rows, rr.probe_lists(700, 700, 31, seed=4), label="training handle")
        ix.free()

    training_twin(cfg, w, pk, calls)


def test_generic_width_handle(hip_lib):
    """rows of 30 and 96 columns, the first no multiple of 4; the PCA map of each scored by both routes"""
    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    for level, k in (("structure", 2), ("atom", 5)):
        index = model.build_index(data, level=level)
        rows = index.rows()[0]
        check_pool(model.engine, index._ix, rows, rr.probe_lists(len(rows), len(rows), 7, seed=1), label="generic " + level)
        res = index.pca(2)
        same_quality(index.map_quality(res, k=k), index.map_quality(res, k=k, route="host"), "generic " + level)
        index.free()


# ---- 7. end to end, the CLI ----

def same_sweep(got, want, label):
    assert got["perplexity"] == want["perplexity"] and got["best_perplexity"] == want["best_perplexity"], label
    for key in ("neighbour_overlap", "trustworthiness", "continuity", "lcmc", "rnx_auc", "kl"):
        assert got[key].tobytes() == want[key].tobytes(), "%s: %s" % (label, key)
    same_quality(got["quality"], want["quality"], label + ": quality")
    assert got["best"]["coords"].tobytes() == want["best"]["coords"].tobytes(), label


def test_map_quality_of_a_model_is_the_host_route_on_its_rows(hip_lib):
    from scann.models import latent_index as li

    cfg, w, data, model = setup(n=4)
    index = model.build_index(data, level="atom")
    rows = index.rows()[0]
    N = len(rows)
    res, emb = model.fit_embedding(index, perplexity=5, iterations=(50, 100))
    dev = model.map_quality(index, emb, k=5)
    print("%d atom rows: trustworthiness %.4f continuity %.4f overlap %.4f" % (N, dev["trustworthiness"], dev["continuity"], dev["neighbour_overlap"]))
    same_quality(dev, index.map_quality(emb, k=5, route="host"), "the index's host route")
    same_quality(dev, li.map_quality_rows_host(rows, emb.coordinates, k=5), "the rows alone")
    same_quality(dev, index.map_quality(res, k=5, graph=(res["neighbor_position"], res["neighbor_dist2"])), "embed's result and its graph")
    same_quality(dev, model.map_quality(data, res["coords"], level="atom", k=5), "data instead of an index")
    for kw in (dict(sample=min(20, N), seed=3), dict(sample=np.array([5, 0, 7], np.int32))):
        part = index.map_quality(emb, k=5, **kw)
        same_quality(part, index.map_quality(emb, k=5, route="host", **kw), "a sample")
        assert part["rank_latent"].tobytes() == dev["rank_latent"][part["position"]].tobytes()
    free0, _ = model.engine.device_memory()
    index.map_quality(emb, k=5)
    assert free0 - model.engine.device_memory()[0] <= 16 << 20                  # the temporary index of the coordinates is gone
    table, best = model.choose_perplexity(index, [5, 10], k=5, iterations=(50, 100))
    assert table["perplexity"] == [5.0, 10.0, "linear"] and len(table["neighbour_overlap"]) == 3 and np.isnan(table["kl"][2])
    assert table["best_perplexity"] == [5.0, 10.0][int(np.argmax(table["neighbour_overlap"][:2]))] == best.perplexity
    same_sweep(table, li.choose_perplexity_rows_host(rows, [5, 10], k=5, iterations=(50, 100))[0], "the rows alone")
    assert table["neighbour_overlap"][0] == dev["neighbour_overlap"] and table["kl"][0] == res["kl"]
    index.free()


def test_cli_prints_the_scores(hip_lib, tmp_path):
    """predict_model.py --embed --map-quality 5 adds the scores to what it prints and pickles; --embed-sweep 5,10 prints the table; the
    other files' bytes are those of a run without the flags"""
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
    r = subprocess.run(cli + ["--embed", "--embed-level", "atom", "--embed-perplexity", "5", "--map-quality", "5", "--project", "2",
                              "--project-level", "atom"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plain = {f: open(out / f, "rb").read() for f in ("ga_scores_homo.pickle", "energy_pre_homo.pickle")}
    listed = set(os.listdir(out))
    assert r.stdout.count("map quality at k = 5: trustworthiness") == 2
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    got = pickle.load(open(out / "embedding_homo.pickle", "rb"))
    same_quality(got["quality"], scann.map_quality(pool, got["coords"], k=5), "the pickled scores of the embedding")
    assert "trustworthiness %.6f" % got["quality"]["trustworthiness"] in r.stdout
    lin = pickle.load(open(out / "projection_homo.pickle", "rb"))
    same_quality(lin["quality"], scann.map_quality(pool, lin["coordinates"], k=5), "the pickled scores of the linear map")
    r = subprocess.run(cli + ["--embed-sweep", "5,10", "--embed-level", "atom", "--map-quality", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"embed_sweep_homo.pickle"}
    want, _ = scann.choose_perplexity(pool, [5, 10], k=5)
    same_sweep(pickle.load(open(out / "embed_sweep_homo.pickle", "rb")), want, "the pickled table")
    assert "best perplexity %g" % want["best_perplexity"] in r.stdout and "linear" in r.stdout and "neighbour overlap" in r.stdout
    r = subprocess.run(cli + ["--map-quality", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--map-quality: needs" in r.stderr
    pool.free()


# ---- 8. bad arguments ----

def test_an_empty_pool_and_errors_name_what_is_wrong(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    empty = eng.index_create(8)
    r = eng.index_ranks(empty, np.zeros((0, 3), np.int32), dist2=True)
    assert r["rank"].shape == (0, 3) and r["dist2"].shape == (0, 3)
    rows = rr.pathological_pool(65, 4)
    pool, foreign = make_index(eng, rows), make_index(other.engine, rows)
    P = _hip._ptr
    probe = rr.probe_lists(65, 65, 3, seed=2)
    out, d2 = np.full((65, 3), 7, np.int32), np.full((65, 3), 7, np.float32)
    q = np.array([1, 65], np.int32)
    bad = probe.copy()
    bad[3, 1] = 65
    low = probe.copy()
    low[0, 2] = -2

    def message():
        return (eng.lib.scann_last_error(eng._h) or b"").decode()

    def call(p=pool, qpos=None, nq=0, pr=probe, m=3, rank=out, dist2=d2):
        return eng.lib.scann_index_ranks(eng._h, None if p is None else p._h, P(qpos), nq, P(pr), m, P(rank), P(dist2))

    free0, _ = eng.device_memory()
    assert call(p=None) == -1 and "scann_index_ranks: null handle or pool" in message()
    assert call(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert call(pr=None) == -1 and "probe is null" in message()
    assert call(rank=None) == -1 and "rank is null" in message()
    for m in (0, 33, -1):
        assert call(m=m) == -1 and "m %d outside 1 .. 32" % m in message()
    assert call(pr=bad) == -1 and "probe[10] = 65 outside -1 .. 64" in message()
    assert call(pr=low) == -1 and "probe[2] = -2 outside -1 .. 64" in message()
    assert call(qpos=q, nq=2) == -1 and "qpos[1] = 65 outside 0 .. 64" in message()
    assert call(qpos=q, nq=-1) == -1 and "nq -1 outside" in message()
    assert (out == 7).all() and (d2 == 7).all() and free0 - eng.device_memory()[0] <= 8 << 20
    assert call() == 0 and call(qpos=q, nq=1) == 0 and call(dist2=None) == 0
    assert out.tobytes() == _hip.ranks_host(rows, probe)["rank"].tobytes()
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError, match="m 33 outside"):
        eng.index_ranks(pool, np.zeros((65, 33), np.int32))
    with pytest.raises(ValueError, match=r"probe\[10\] = 65"):
        eng.index_ranks(pool, bad)
    with pytest.raises(ValueError, match=r"qpos\[1\] = 65"):
        eng.index_ranks(pool, probe[:2], q)
    lat = model.build_index(data, level="atom")
    N = len(lat)
    coords = np.random.default_rng(0).standard_normal((N, 2)).astype(np.float32)
    for kw, word in ((dict(k=0), "k must be"), (dict(k=32), "k must be"), (dict(route="gpu"), "route"), (dict(sample=0), "sample"),
                     (dict(sample=[N]), "sample"), (dict(sample=N + 1), "only"), (dict(seed=-1), "seed")):
        with pytest.raises(ValueError, match=word):
            lat.map_quality(coords, **dict(dict(k=3), **kw))
    with pytest.raises(ValueError, match="one row per row"):
        lat.map_quality(coords[:-1], k=3)
    with pytest.raises(ValueError, match="non-finite"):
        lat.map_quality(np.where(np.arange(N)[:, None] == 2, np.inf, coords), k=3)
    with pytest.raises(ValueError):
        other.map_quality(lat, coords, k=3)  # another model's index
    with pytest.raises(ValueError, match="perplexities"):
        model.choose_perplexity(data, [10, 5])
    with pytest.raises(ValueError, match="level"):
        model.choose_perplexity(data, [5, 10], level="bond")
    good = lat.map_quality(coords, k=3)                                          # and the next good call succeeds
    assert good["k"] == 3 and 0.0 <= good["neighbour_overlap"] <= 1.0
    for ix in (empty, pool, foreign, lat):
        ix.free()

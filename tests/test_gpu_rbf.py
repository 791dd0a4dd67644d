"""GPU tests of the Gaussian landmark features and the kernel head (scann_index_rbf_features / scann_rbf_head_batch through
Engine.index_rbf_features, rbf_head_batch; LatentIndex.fit_kernel_head, HipModel.fit_kernel_head / predict_kernel_head).  Every
comparison of a device result with a twin is an equality of bit patterns (a NaN equals a NaN).

1. Engine.index_rbf_features == the twin scann_rbf_features_host: N either side of the 128-row tile, m either side of the 64-landmark
   tile, dim either side of the 32-column slab and no multiple of 4, the smallest and the largest widths; planted NaN / inf / far rows;
   two storage chunks of the pool and of the output; one add or many; a repeat; ids and atoms; and, independent of the twin, the weight
   chain applied to Engine.index_query's distances.
2. Engine.rbf_head_batch on the qm9 and mp2018 fixtures at both levels == read_output -> rbf_features_host -> project_host and one fp32
   add each; a generic width; an exact-fp32 handle.  3. End to end against the host route (tests/rbf_ref.py), the planted data with its
   0.9 / 0.1 assertion among them.  4. Non-interference.  5. Errors name the argument; the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of the exact-fp32 test
    for p in (os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, p)

import head_ref  # noqa: E402
import pca_ref  # noqa: E402
import rbf_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import _bits, make_index, random_rows, setup, training_twin, untouched  # noqa: E402
from test_gpu_head import random_eval_head, targets_for  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def landmarks_for(rows, m, seed=0):
    """m landmarks among and around finite rows of the pool (a landmark on a row: distance 0, weight 1), and a gamma that spreads
    u = dist2 gamma over the chain's range: the median distance gets u = 6"""
    from scann import _hip

    rng = np.random.default_rng(seed + m)
    ok = np.nonzero(np.isfinite(rows).all(1) & (np.abs(rows) < 1e10).all(1))[0]
    Z = rows[ok[rng.integers(0, len(ok), m)]].copy()
    Z[1::2] += rng.standard_normal(Z[1::2].shape).astype(np.float32) * np.float32(0.5)
    d2 = _hip.knn_dist2_matrix(rows[ok[:64]], Z)
    med = float(np.median(d2[d2 > 0])) if (d2 > 0).any() else 1.0
    return Z, float(np.float32(6.0 / med))


def features(eng, ix, Z, gamma):
    """(phi [N, m], ids, atoms) of Engine.index_rbf_features, the feature index freed"""
    out = eng.index_rbf_features(ix, Z, gamma)
    try:
        assert len(out) == len(ix) and out.dim == len(Z)
        return eng.index_read(out)
    finally:
        out.free()


@pytest.fixture(scope="module")
def two_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns"""
    rows = random_rows(17000, 1024)
    ix = make_index(engine, rows)
    yield rows, ix
    ix.free()


# ---- 1. the features ----

FEATURE_SHAPES = [(1, 1, 1), (127, 3, 5), (128, 16, 64), (129, 128, 65), (1000, 130, 257), (300, 1024, 1024)]


@pytest.mark.parametrize("N,dim,m", FEATURE_SHAPES, ids=["N%d_d%d_m%d" % s for s in FEATURE_SHAPES])
def test_features_equal_the_host_twin(engine, N, dim, m):
    from scann import _hip

    rows = random_rows(N, dim)
    Z, gamma = landmarks_for(rows, m)
    ix = make_index(engine, rows)
    try:
        phi, ids, atoms = features(engine, ix, Z, gamma)
        again = features(engine, ix, Z, gamma)[0]
    finally:
        ix.free()
    want = _hip.rbf_features_host(rows, Z, gamma)
    print("N %d dim %d m %d: gamma %.3g, features in [%.3g, %.3g], %d are 1, %d are 0, %d differ" % (
        N, dim, m, gamma, phi.min(), phi.max(), int((phi == 1).sum()), int((phi == 0).sum()), int((_bits(phi) != _bits(want)).sum())))
    pca_ref.same(phi, want, "N %d dim %d m %d" % (N, dim, m))
    pca_ref.same(again, phi, "repeat")
    assert np.array_equal(ids, np.arange(N)) and np.all(atoms == -1) and (phi == 1).any()


def test_features_of_planted_rows(engine):
    from scann import _hip

    rows = random_rows(700, 130, seed=12)
    Z, gamma = landmarks_for(rows, 70)
    rows[13, 129] = np.nan
    rows[300, 128] = np.inf
    rows[301, 0] = -np.inf
    rows[301, 5] = np.nan
    rows[500] = np.float32(3e19)  # finite: every distance overflows to +inf, every feature is 0
    rows[501, 64] = np.float32(1e6)  # far, not overflowing: u >= 126
    ids, atoms = np.arange(700, dtype=np.int64) * 5 + 2, (np.arange(700) % 11).astype(np.int32)
    ix = engine.index_create(130)
    try:
        engine.index_add(ix, rows, ids, atoms)
        phi, got_ids, got_atoms = features(engine, ix, Z, gamma)
    finally:
        ix.free()
    pca_ref.same(phi, _hip.rbf_features_host(rows, Z, gamma), "planted")
    assert np.isnan(phi[[13, 300, 301]]).all() and not phi[[500, 501]].any()
    assert not np.isnan(np.delete(phi, [13, 300, 301], axis=0)).any() and np.nanmax(phi) <= 1 and np.nanmin(phi) >= 0
    assert np.array_equal(got_ids, ids) and np.array_equal(got_atoms, atoms)  # ids and atoms carried over


def test_features_over_two_pool_chunks(engine, two_chunks):
    from scann import _hip

    rows, ix = two_chunks
    Z, gamma = landmarks_for(rows, 8)
    Z[0], Z[1] = rows[16383], rows[16384]  # a landmark on either side of the chunk boundary
    phi = features(engine, ix, Z, gamma)[0]
    pca_ref.same(phi, _hip.rbf_features_host(rows, Z, gamma), "two pool chunks")
    assert phi[16383, 0] == 1 and phi[16384, 1] == 1


def test_features_whose_output_crosses_a_chunk(engine):
    """17,000 x 4 -> 17,000 x 1,024: the feature index's chunks hold 16,384 rows"""
    from scann import _hip

    rows = random_rows(17000, 4)
    Z, gamma = landmarks_for(rows, 1024)
    ix = make_index(engine, rows)
    try:
        phi = features(engine, ix, Z, gamma)[0]
    finally:
        ix.free()
    pca_ref.same(phi, _hip.rbf_features_host(rows, Z, gamma), "two output chunks")


def test_features_do_not_depend_on_how_the_pool_was_built(engine):
    dim, N = 130, 3000
    rows = random_rows(N, dim, seed=9)
    Z, gamma = landmarks_for(rows, 100)
    one, many = engine.index_create(dim), engine.index_create(dim)
    try:
        engine.index_add(one, rows)
        at = 0
        for step in [1, 63, 64, 65, 7, 1000, 3, 500, 255, 257]:
            engine.index_add(many, rows[at:at + step])
            at += step
        engine.index_add(many, rows[at:])
        a, b = features(engine, one, Z, gamma), features(engine, many, Z, gamma)
    finally:
        one.free()
        many.free()
    pca_ref.same(b[0], a[0], "many adds")
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_features_independent_of_the_twin(engine):
    """N = 20: the features are the weight chain applied to Engine.index_query's distances of the landmarks to all 20 rows, put back in
    position order"""
    from scann import _hip

    rows = random_rows(20, 37, seed=3)
    Z, gamma = landmarks_for(rows, 9)
    ix = make_index(engine, rows)
    try:
        phi = features(engine, ix, Z, gamma)[0]
        q = engine.index_query(ix, Z, 20)
    finally:
        ix.free()
    want = np.empty((20, 9), np.float32)
    for c in range(9):
        assert sorted(q["position"][c].tolist()) == list(range(20))
        want[q["position"][c], c] = _hip.rbf_weight(q["dist2"][c], gamma)
    pca_ref.same(phi, want, "the weight of the search's distances")


def test_features_of_an_empty_pool(engine):
    ix = engine.index_create(8)
    try:
        out = engine.index_rbf_features(ix, np.ones((3, 8), np.float32), 0.5)
        assert len(out) == 0 and out.dim == 3
        out.free()
    finally:
        ix.free()


# ---- 2. the kernel head behind a forward ----

def check_rbf_head_batch(model, data, label):
    """rbf_head_batch == read_output -> rbf_features_host -> project_host with (mean, W) and with (mean, V, S[k]) plus one fp32 add each;
    y and ga those of a plain forward"""
    from scann import _hip

    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(data))
    eng.set_outputs(after_lc=True, bf_property=True)
    try:
        eng.forward_resident(rb)
        y, ga = eng.download(rb)
        level_rows = {"structure": eng.read_output(rb, _hip.OUT_BF_PROPERTY), "atom": eng.read_output(rb, _hip.OUT_AFTER_LC)}
    finally:
        eng.set_outputs()
    for level in ("structure", "atom"):
        lvl, rows = _hip.KNN_LEVELS[level], level_rows[level]
        K, m, mm = 3, 7, 5
        Z, gamma = landmarks_for(rows, m, seed=len(rows))
        h = random_eval_head(m, K, mm, seed=m + K)
        got = eng.rbf_head_batch(rb, lvl, Z, gamma, h["mean"], h["tmean"], h["weights"], h["components"], h["scale"], h["lev0"])
        phi = _hip.rbf_features_host(rows, Z, gamma)
        pca_ref.same(got["phi"], phi, "%s %s phi" % (label, level))
        w = _hip.project_host(phi, h["mean"], h["weights"])
        pca_ref.same(got["pred"], (h["tmean"][None, :] + w["coords"]).astype(np.float32), "%s %s pred" % (label, level))
        for k in range(K):
            md2 = _hip.project_host(phi, h["mean"], h["components"], h["scale"][k])["md2"]
            pca_ref.same(np.ascontiguousarray(got["lev"][:, k]), (h["lev0"] + md2).astype(np.float32), "%s %s lev %d" % (label, level, k))
        pca_ref.same(got["y"], y, "y")
        pca_ref.same(got["ga"], ga, "ga")
        bare = eng.rbf_head_batch(rb, lvl, Z, gamma, h["mean"], h["tmean"], h["weights"], h["components"], h["scale"], h["lev0"], want_phi=False)
        assert "phi" not in bare
        pca_ref.same(bare["pred"], got["pred"], "without phi")
        print("%s %s: %d rows of %d columns, phi in [%.3g, %.3g]" % (label, level, len(rows), rows.shape[1], phi.min(), phi.max()))
    rb.free()


@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_rbf_head_batch_is_features_two_projections_and_an_add(hip_lib, kind):
    cfg, w, data, model = setup(kind=kind, n=24 if kind == "mp2018" else 40, seed=0)
    check_rbf_head_batch(model, data, kind)


def test_rbf_head_batch_on_a_generic_width_handle(hip_lib):
    """rows of 30 and 96 columns, the first no multiple of 4"""
    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    check_rbf_head_batch(model, data, "generic")


def child_scenario():
    cfg, w, data, model = setup(n=10, seed=3)
    check_rbf_head_batch(model, data, "child")
    return model.engine.exact_reruns()


def test_rbf_head_batch_on_an_exact_fp32_handle(hip_lib):
    """a handle whose forwards run exact-fp32 (SCANN_EXACT=1): a fresh process"""
    e = dict(os.environ)
    e["SCANN_EXACT"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 3. end to end ----

E2E = {"qm9": 64, "mp2018": 24}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_fit_kernel_head_is_the_host_route_on_the_models_rows(hip_lib, kind, level, tmp_path):
    from scann import _hip
    from scann.models import LatentKernelHead

    n = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n, seed=0)
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    rows, ids, atoms = index.rows()
    t = targets_for(rows, 2, seed=4)
    t[3, 1] = np.nan  # unlabelled
    m = 12
    got, head = model.fit_kernel_head(index, t, landmarks=m, names=["a", "b"])
    want, head_w = rbf_ref.host_fit(rows, t, landmarks=m, names=["a", "b"], level=level, ids=ids, atoms=atoms)
    print("%s %s: n_rows %d, bandwidth %.4g of %s, covering radius %.4g, l2 %s, loo_r2 %s" % (
        kind, level, got["n_rows"], got["bandwidth"], got["bandwidth_path"]["bandwidth"], got["covering_radius"], got["l2"], got["loo_r2"]))
    rbf_ref.same_fit(got, head, want, head_w, "%s %s" % (kind, level))
    assert got["n_rows"] == len(rows) - 1 and got["names"] == ["a", "b"] and np.isnan(got["loo_prediction"][3]).all()
    # predict_kernel_head right after, padded and packed: the head on the rows of the index
    a = model.predict_kernel_head(data, head, batch_size=16)
    pk = model.predict_kernel_head(_hip.pack_inputs(data), head, batch_size=16)
    y, ga = model.predict(data)
    assert np.array_equal(_bits(a["y"]), _bits(y)) and np.array_equal(_bits(pk["y"]), _bits(y)) and np.array_equal(_bits(a["ga"]), _bits(ga))
    assert sorted(pk) == ["ga", "leverage", "prediction", "std", "support", "y"]
    phi = _hip.rbf_features_host(rows, head.landmarks, head.gamma)
    proj = _hip.project_host(phi, head.head.mean, head.head.weights)
    pca_ref.same(pk["prediction"], (head.head.tmean[None, :] + proj["coords"]).astype(np.float32), "prediction")
    pca_ref.same(pk["support"], phi.max(axis=1), "support")
    assert pk["std"].shape == pk["prediction"].shape == (len(rows), 2) and np.all(pk["std"] >= np.sqrt(head.head.sigma2).astype(np.float32)[None, :])
    assert np.all(pk["leverage"] >= head.head.lev0) and np.all(pk["support"][got["landmark_position"]] == 1)
    for key in ("prediction", "std", "leverage", "support"):
        pca_ref.same(a[key], pk[key] if level == "structure" else _hip.repad_atoms(pk[key], data["atom_mask"], 0), "padded " + key)
    # data instead of an index (at atom level one array of targets per structure); explicit positions and bandwidth; save and load
    if level == "atom":
        counts = np.asarray(data["atom_mask"]).reshape(np.shape(data["neighbors"])[:2]).astype(bool).sum(1)
        per = np.split(t, np.cumsum(counts)[:-1])
        direct, _ = model.fit_kernel_head(data, per, level="atom", landmarks=m, batch_size=16, names=["a", "b"])
    else:
        direct, _ = model.fit_kernel_head(data, t, landmarks=m, batch_size=16, names=["a", "b"])
    pca_ref.same(direct["loo_prediction"], got["loo_prediction"], "direct")
    pos = got["landmark_position"][::-1].copy()
    by_pos = index.fit_kernel_head(t, landmarks=pos, bandwidth=[got["bandwidth"], 2 * got["bandwidth"]], names=["a", "b"])
    by_pos_w = rbf_ref.host_fit(rows, t, landmarks=pos, bandwidth=[got["bandwidth"], 2 * got["bandwidth"]], names=["a", "b"], level=level, ids=ids, atoms=atoms)
    rbf_ref.same_fit(by_pos[0], by_pos[1], by_pos_w[0], by_pos_w[1], "explicit positions")
    assert by_pos[0]["covering_radius"] == got["covering_radius"]
    head.save(str(tmp_path / "kh.npz"))
    back = LatentKernelHead.load(model, str(tmp_path / "kh.npz"))
    pca_ref.same(model.predict_kernel_head(data, back, batch_size=16)["std"], a["std"], "loaded head")
    index.free()


def test_fit_kernel_head_on_planted_rows(hip_lib):
    """a structure-level LatentIndex filled by add_rows with planted(600, dense_out, 3, 0): the device's numbers are the host route's, the
    kernel head reads the target (loo_r2 >= 0.9) and the linear head does not (<= 0.1)"""
    from scann.models import LatentIndex

    cfg, w, data, model = setup(n=4)
    rows, t = rbf_ref.planted(600, cfg["model"]["dense_out"], 3, 0)
    index = LatentIndex(model, "structure").add_rows(rows)
    got, head = index.fit_kernel_head(t, landmarks=64)
    linear, _ = index.fit_head(t)
    free0, _ = model.engine.device_memory()
    again, head_a = index.fit_kernel_head(t, landmarks=64)
    assert free0 - model.engine.device_memory()[0] <= 16 << 20  # the temporary feature indices are freed: their chunks are back in the block cache
    rbf_ref.same_fit(again, head_a, got, head, "repeat")
    want, head_w = rbf_ref.host_fit(rows, t, landmarks=64)
    print("planted: kernel head loo_r2 %.4f at h = %.3g (path %s), linear head loo_r2 %.4f" % (
        got["loo_r2"][0], got["bandwidth"], np.round(got["bandwidth_path"]["loo_r2"][:, 0], 4), linear["loo_r2"][0]))
    rbf_ref.same_fit(got, head, want, head_w, "planted")
    pca_ref.same(linear["loo_r2"], head_ref.host_fit(rows, t)[0]["loo_r2"], "the linear head")
    assert got["loo_r2"][0] >= 0.9
    assert linear["loo_r2"][0] <= 0.1
    index.free()


# ---- 4. state ----

def test_nothing_else_changes(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool, rb = u.eng, u.pool, u.rb
        Z, gamma = landmarks_for(u.rows[0], 70)
        first = features(eng, pool, Z, gamma)[0]
        u.repeat(lambda: features(eng, pool, Z, gamma)[0], lambda r: pca_ref.same(r, first, "repeat"), 5, 16 << 20)
        u.check()
        # rbf_head_batch: y is the plain forward's; the selection is put back
        h = random_eval_head(6, 2, 4, seed=1)
        Zs = np.random.default_rng(0).standard_normal((6, 128)).astype(np.float32)
        r = eng.rbf_head_batch(rb, _hip.OUT_BF_PROPERTY, Zs, 0.01, h["mean"], h["tmean"], h["weights"], h["components"], h["scale"], h["lev0"])
        assert np.array_equal(_bits(r["y"]), _bits(u.y_first))
        u.reforward()


def test_training_handle(hip_lib):
    """after two training steps the calls on the training handle equal the host twin's and an inference handle's, and weights, gradients
    and the following (deterministic) step -- the Adam state entered it -- are those of a twin that never made the calls"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows = random_rows(900, 128, seed=8)
    Z, gamma = landmarks_for(rows, 40)
    h = random_eval_head(5, 2, 4, seed=2)
    Zs = np.random.default_rng(1).standard_normal((5, 128)).astype(np.float32)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, rows)
        pca_ref.same(features(eng, ix, Z, gamma)[0], _hip.rbf_features_host(rows, Z, gamma), "training handle")
        ix.free()
        inf_model, rb2 = inference()
        inf = inf_model.engine
        for level in (_hip.OUT_BF_PROPERTY, _hip.OUT_AFTER_LC):
            hb = [e.rbf_head_batch(b, level, Zs, 0.01, h["mean"], h["tmean"], h["weights"], h["components"], h["scale"], h["lev0"])
                  for e, b in ((eng, rb), (inf, rb2))]
            for key in hb[0]:
                pca_ref.same(hb[0][key], hb[1][key], "training against inference handle, " + key)

    training_twin(cfg, w, pk, calls)


# ---- 5. errors, the CLI ----

def test_errors_name_what_is_wrong(hip_lib):
    from scann import _hip
    from scann.models import LatentIndex

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows = random_rows(5, 4, seed=0)
    Z = rows[:2].copy()
    pool, foreign = make_index(eng, rows), make_index(other.engine, rows)
    out, wide, full, far = eng.index_create(2), eng.index_create(3), make_index(eng, rows[:, :2].copy()), other.engine.index_create(2)
    P = _hip._ptr

    def feat(p=pool, Z=Z, m=2, gamma=0.5, o=out):
        return eng.lib.scann_index_rbf_features(eng._h, None if p is None else p._h, P(Z), m, gamma, None if o is None else o._h)

    def message(e=eng):
        return (eng.lib.scann_last_error(e._h) or b"").decode()

    def with_bad(a, at, v=np.nan):
        b = a.copy()
        b.reshape(-1)[at] = v
        return b

    free0, _ = eng.device_memory()
    assert feat(p=None) == -1 and "null" in message()
    assert feat(o=None) == -1 and "out is null" in message()
    assert feat(Z=None) == -1 and "landmarks is null" in message()
    assert feat(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert feat(o=far) == -1 and "out belongs to another handle" in message()
    assert feat(o=pool, m=4, Z=np.zeros((4, 4), np.float32)) == -1 and "out is the pool itself" in message()
    assert feat(o=full) == -1 and "out is not empty" in message() and "5 rows" in message()
    assert feat(o=wide) == -1 and "out holds rows of 3 columns, m is 2" in message()
    assert feat(m=0) == -1 and "m 0 outside 1 .. 1024" in message()
    assert feat(m=1025) == -1 and "m 1025 outside 1 .. 1024" in message()
    assert feat(Z=with_bad(Z, 6)) == -1 and "landmarks hold a non-finite value (landmark 1, column 2)" in message()
    assert feat(Z=with_bad(Z, 3, np.inf)) == -1 and "(landmark 0, column 3)" in message()
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert feat(gamma=g) == -1 and "gamma must be finite and > 0" in message(), g
    assert len(out) == 0 and len(full) == 5
    rb = eng.upload(_hip.pack_inputs(data))
    h = random_eval_head(6, 2, 3, seed=0)
    Zs = np.random.default_rng(0).standard_normal((6, 128)).astype(np.float32)
    pred = np.full((4, 2), 7, np.float32)

    def batch(level=_hip.OUT_BF_PROPERTY, b=rb, Z=Zs, m=6, gamma=0.01, K=2, mm=3, pred=pred, **kw):
        a = dict(h)
        a.update(kw)
        return eng.lib.scann_rbf_head_batch(eng._h, None if b is None else b._h, level, P(Z), m, gamma, P(a["mean"]), P(a["tmean"]), P(a["weights"]), K,
                                            P(a["components"]), mm, P(a["scale"]), float(a["lev0"]), None, None, P(pred),
                                            P(np.zeros((4, 2), np.float32)), None)

    assert batch(b=None) == -1 and "null handle or batch" in message()
    assert batch(level=9) == -1 and "level must be" in message() and "got 9" in message()
    assert batch(Z=None) == -1 and "landmarks is null" in message()
    assert batch(m=0) == -1 and "m 0 outside 1 .. 1024" in message()
    assert batch(Z=with_bad(Zs, 130)) == -1 and "(landmark 1, column 2)" in message()
    assert batch(gamma=0.0) == -1 and "gamma must be finite and > 0" in message()
    assert batch(K=17) == -1 and "K 17 outside 1 .. 16" in message()
    assert batch(mm=7) == -1 and "m 7 outside 1 .. 6" in message()
    assert batch(weights=None) == -1 and "weights is null" in message()
    assert batch(pred=None) == -1 and "pred is null" in message()
    assert batch(weights=with_bad(h["weights"], 7)) == -1 and "weights hold a non-finite value (target 1)" in message()
    assert batch(scale=with_bad(h["scale"], 0)) == -1 and "scale holds a non-finite value (target 0)" in message()
    assert batch(lev0=np.nan) == -1 and "lev0 is not finite" in message()
    # nothing was written, nothing stays allocated
    assert np.all(pred == 7) and free0 - eng.device_memory()[0] <= 8 << 20
    assert feat() == 0 and len(out) == 5 and batch() == 0
    rb.free()
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError, match="landmarks"):
        eng.index_rbf_features(pool, np.zeros((2, 5), np.float32), 0.5)
    with pytest.raises(ValueError, match="gamma"):
        eng.index_rbf_features(pool, Z, 0.0)
    lat = model.build_index(data)
    for bad in (np.zeros(3), np.zeros((4, 17)), "x"):
        with pytest.raises(ValueError):
            lat.fit_kernel_head(bad, landmarks=2)
    for kw in (dict(l2="cv"), dict(bandwidth="cv"), dict(bandwidth=0.0), dict(bandwidth=[1.0] * 9), dict(landmarks=0), dict(landmarks=1025),
               dict(landmarks=np.array([0, 0])), dict(landmarks=np.array([0, 4])), dict(names=["a", "b"])):
        with pytest.raises(ValueError):
            lat.fit_kernel_head(np.arange(4, dtype=np.float32), **dict(dict(landmarks=2), **kw))
    with pytest.raises(ValueError, match="more usable rows than landmarks"):
        lat.fit_kernel_head(np.arange(4, dtype=np.float32), landmarks=4)
    same = LatentIndex(model, "structure").add_rows(np.ones((6, 128), np.float32))
    with pytest.raises(ValueError, match="covering radius"):
        same.fit_kernel_head(np.arange(6, dtype=np.float32), landmarks=1)
    with pytest.raises(ValueError):
        other.fit_kernel_head(lat, np.zeros(4), landmarks=2)  # another model's index
    with pytest.raises(ValueError):
        model.predict_kernel_head(data, "a head")
    for ix in (pool, foreign, out, wide, full, far, lat, same):
        ix.free()


def test_cli_fits_and_applies_a_kernel_head(hip_lib, tmp_path):
    """predict_model.py --fit-kernel-head writes kernel_head_<target>.pickle and, with --kernel-head-out, the head; --kernel-head applies
    it; the other files' bytes are those of a run without the flags"""
    import yaml

    from scann.models import SCANN, LatentKernelHead
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
    t = np.random.default_rng(0).standard_normal((n, 2)).astype(np.float32)
    np.save(tmp_path / "t.npy", t)
    cli = [sys.executable, os.path.join(ROOT, "predict_model.py"), str(out)]
    r = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plain = {f: open(out / f, "rb").read() for f in ("ga_scores_homo.pickle", "energy_pre_homo.pickle")}
    listed = set(os.listdir(out))
    r = subprocess.run(cli + ["--fit-kernel-head", str(tmp_path / "t.npy"), "--landmarks", "6", "--kernel-head-out", str(tmp_path / "kh.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"kernel_head_homo.pickle"}
    got = pickle.load(open(out / "kernel_head_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="structure", ids=data.indexes)
    want, head = scann.fit_kernel_head(pool, t, landmarks=6)
    assert sorted(got) == sorted(list(want) + ["id", "atom"])
    for key in ("l2", "loo_rmse", "loo_r2", "loo_prediction", "weights", "landmark_position", "landmark_id"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert got["bandwidth"] == want["bandwidth"] and "loo_rmse" in r.stdout and "target_1" in r.stdout and "n_rows %d" % n in r.stdout
    saved = LatentKernelHead.load(scann.model, str(tmp_path / "kh.npz"))
    pca_ref.same(saved.landmarks, head.landmarks, "landmarks")
    assert saved.gamma == head.gamma
    for key in rbf_ref.HEAD_ARRAYS:
        pca_ref.same(getattr(saved.head, key), getattr(head.head, key), key)
    r = subprocess.run(cli + ["--kernel-head", str(tmp_path / "kh.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    per = pickle.load(open(out / "kernel_head_homo.pickle", "rb"))
    assert len(per) == n and sorted(per[0]) == ["leverage", "predict_property", "prediction", "std", "support"] and per[0]["prediction"].shape == (2,)
    inputs, _ = data[0]
    first = scann.predict_kernel_head(inputs, head)
    assert np.array_equal(per[0]["prediction"], first["prediction"][0]) and np.array_equal(per[0]["std"], first["std"][0])
    assert per[0]["support"] == first["support"][0]
    pool.free()


if __name__ == "__main__":
    reruns = child_scenario()
    print("child ok, exact re-runs %d" % reruns)

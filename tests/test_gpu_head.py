"""GPU tests of the readout head on a latent index (scann_index_fit_moments / scann_index_ridge_loo / scann_head_batch through
Engine.index_fit_moments, index_ridge_loo, head_batch; LatentIndex.fit_head, HipModel.fit_head / predict_head).  Every comparison of a
device result is an equality of bit patterns (a NaN equals a NaN).

1. Engine.index_fit_moments == the host twin of scann_index_moments on the augmented matrix [rows | t]: N either side of the slabs, dim
   from 1 to the maximum, K 1 .. 3; planted NaN / inf rows and NaN targets, a constant target; two storage chunks; one add or many.
2. Engine.index_ridge_loo == the twin scann_ridge_loo_host: N either side of the 128-row tile, dim 1 .. 1,024, m < dim and m = dim, L 1, 5,
   32, K 1, 3, 16 -- L (K + 1) above one 64-column pass among them --, the planted +inf, resid, two chunks, a repeat; independent of the
   twin: with B = 0 sse_fit is the block-ordered sum of (t - tmean)^2, and dof the block-ordered sum of lev0 + Engine.index_project's md2.
3. Engine.head_batch on the qm9 and mp2018 fixtures at both levels == two Engine.project_batch calls and one fp32 add each; a generic
   width; an exact-fp32 handle.  4. End to end against the host route.  5. Non-interference.  6. Errors name the argument; the CLI."""
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
import scann_oracle as so  # noqa: E402
from analysis_checks import (SUBNORMAL, _bits, make_index, random_rows, scan_edge_rows, setup, subnormal_column, training_twin,  # noqa: E402
                             untouched)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def targets_for(rows, K, seed=0):
    """targets of very different scale and offset, linear in the rows plus noise"""
    rng = np.random.default_rng(seed + 17 * K)
    x = np.nan_to_num(rows.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    t = x @ (rng.standard_normal((rows.shape[1], K)) / np.sqrt(rows.shape[1])) + rng.standard_normal((len(rows), K))
    return (t * rng.uniform(0.01, 100, K) + rng.standard_normal(K) * 3).astype(np.float32)


@pytest.fixture(scope="module")
def two_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns"""
    rows = random_rows(17000, 1024)
    ix = make_index(engine, rows)
    yield rows, ix
    ix.free()


# ---- 1. the augmented moments ----

MOMENT_SHAPES = [(2, 3, 1), (33, 16, 2), (127, 128, 1), (129, 130, 3), (5000, 130, 2), (600, 1024, 1)]


@pytest.mark.parametrize("N,dim,K", MOMENT_SHAPES, ids=["N%d_d%d_K%d" % c for c in MOMENT_SHAPES])
def test_fit_moments_equal_the_host_twin(engine, N, dim, K):
    from scann import _hip

    rows = random_rows(N, dim)
    t = targets_for(rows, K)
    want = _hip.moments_host(head_ref.augmented(rows, t))
    ix = make_index(engine, rows)
    try:
        got = engine.index_fit_moments(ix, t)
        again = engine.index_fit_moments(ix, t if K > 1 else t[:, 0])
        plain = engine.index_moments(ix)
    finally:
        ix.free()
    print("N %d dim %d K %d: n %d bits %d, %d cov values differ" % (N, dim, K, got["n"], got["bits"], int((got["cov"].view(np.uint64) != want["cov"].view(np.uint64)).sum())))
    pca_ref.same_moments(got, want, "N %d dim %d K %d" % (N, dim, K))
    pca_ref.same_moments(again, got, "repeat")
    assert np.array_equal(got["cov"], got["cov"].T) and got["cov"].shape == (dim + K, dim + K)
    pca_ref.same(np.ascontiguousarray(got["cov"][:dim, :dim]), plain["cov"], "the X-X block is scann_index_moments' covariance")


def test_fit_moments_of_planted_rows(engine):
    from scann import _hip

    rows = random_rows(700, 130, seed=12)
    t = targets_for(rows, 3, seed=1)
    rows[13, 129] = np.nan
    rows[300, 128] = np.inf
    t[5, 0] = np.nan  # unlabelled
    t[699, 2] = np.nan
    t[44, 1] = np.inf
    t[:, 1][np.isfinite(t[:, 1])] = -7.25  # a constant target: its variance is exactly 0
    ix = make_index(engine, rows)
    try:
        got = engine.index_fit_moments(ix, t)
    finally:
        ix.free()
    aug = head_ref.augmented(rows, t)
    pca_ref.same_moments(got, _hip.moments_host(aug), "planted")
    pca_ref.same_moments(got, pca_ref.moments(aug), "planted, NumPy")
    assert got["n"] == 695 and not got["cov"][131].any() and got["mean"][131] == -7.25


def test_fit_moments_at_the_edges_of_the_eligibility_scan(engine):
    """the rows' edges, and the targets' own: six targets, so that lanes 4 and 5 of a row's eight hold one each; NaN in the last of them, a
    column of subnormals among them"""
    from scann import _hip

    for label, rows in scan_edge_rows():
        N, dim = rows.shape
        t = targets_for(rows, 6, seed=3)
        t[:, 2] = subnormal_column(np.random.default_rng(N), N)
        ix = make_index(engine, rows)
        try:
            if N < 2:  # a covariance needs two rows: the twin refuses the index, and the device does once its scan has counted the one
                with pytest.raises(ValueError, match="at least 2 rows"):
                    _hip.moments_host(head_ref.augmented(rows, t))
                with pytest.raises(_hip.ScannHipError, match="has 1 among its 1"):
                    engine.index_fit_moments(ix, t)
                continue
            t[2, 5] = np.nan
            got = engine.index_fit_moments(ix, t)
        finally:
            ix.free()
        pca_ref.same_moments(got, _hip.moments_host(head_ref.augmented(rows, t)), label)
        assert got["n"] == np.isfinite(rows).all(axis=1).sum() - 1, label
        assert 0 < got["mean"][dim + 2] < 400 * SUBNORMAL and got["col_exp"][dim + 2] < -125, label


def test_fit_moments_over_two_chunks(engine, two_chunks):
    rows, ix = two_chunks
    t = targets_for(rows, 1, seed=2)
    t[16390, 0] = np.nan
    got = engine.index_fit_moments(ix, t)
    only = list(range(4)) + list(range(1020, 1025))
    want = pca_ref.moments(head_ref.augmented(rows, t), only=only)
    assert got["n"] == 16999 and got["bits"] == 23
    pca_ref.same(got["mean"], want["mean"], "mean")
    pca_ref.same(got["col_exp"], want["col_exp"], "col_exp")
    pca_ref.same(got["cov"][only], want["cov"], "cov rows")
    assert np.array_equal(got["cov"], got["cov"].T)


def test_fit_moments_do_not_depend_on_how_the_index_was_built(engine):
    dim, N = 130, 3000
    rows = random_rows(N, dim, seed=9)
    t = targets_for(rows, 2, seed=9)
    one, many = engine.index_create(dim), engine.index_create(dim)
    try:
        engine.index_add(one, rows)
        at = 0
        for step in [1, 63, 64, 65, 7, 1000, 3, 500, 255, 257]:
            engine.index_add(many, rows[at:at + step])
            at += step
        engine.index_add(many, rows[at:])
        pca_ref.same_moments(engine.index_fit_moments(many, t), engine.index_fit_moments(one, t), "many adds")
    finally:
        one.free()
        many.free()


# ---- 2. the leave-one-out pass ----

# (N, dim, m, L, K)
LOO_SHAPES = [(127, 1, 1, 1, 1), (128, 16, 16, 5, 3), (129, 16, 7, 32, 16), (257, 128, 128, 5, 3), (1000, 130, 65, 32, 1), (1000, 128, 33, 1, 16),
              (600, 1024, 40, 5, 3)]


def check_loo(eng, ix, args, resid_l, label):
    from scann import _hip

    got = eng.index_ridge_loo(ix, *args[1:], resid_l)
    want = _hip.ridge_loo_host(*args, resid_l)
    print("%s: n %d, sse[0] %s" % (label, got["n"], got["sse"][0][:2]))
    head_ref.same_loo(got, want, label)
    return got


@pytest.mark.parametrize("shape", LOO_SHAPES, ids=["N%d_d%d_m%d_L%d_K%d" % s for s in LOO_SHAPES])
def test_ridge_loo_equals_the_host_twin(engine, shape):
    N, dim, m, L, K = shape
    args = list(head_ref.random_head(*shape, seed=2))
    rows, t = args[0], args[1]
    resid_l = (np.arange(K) % L).astype(np.int32)
    if K > 1:
        resid_l[1] = -1
    ix = make_index(engine, rows)
    try:
        got = check_loo(engine, ix, args, resid_l, "plain")
        head_ref.same_loo(engine.index_ridge_loo(ix, *args[1:], resid_l), got, "repeat")
        head_ref.same_loo(engine.index_ridge_loo(ix, *args[1:]), {k: v for k, v in got.items() if k != "resid"}, "no resid")
    finally:
        ix.free()
    # planted: NaN / inf rows, unlabelled rows, a strength whose leverage passes 1
    rows[5, dim - 1] = np.nan
    rows[N - 1, 0] = np.inf
    t[7, 0] = np.nan
    t[N - 3, K - 1] = np.nan
    args[5] = args[5].copy()
    args[5][L - 1] *= np.float32(4000)
    ix = make_index(engine, rows)
    try:
        got = check_loo(engine, ix, args, resid_l, "planted")
    finally:
        ix.free()
    assert got["n"] == N - 4 and np.isinf(got["sse"][L - 1]).all() and np.isnan(got["resid"][[5, 7, N - 3, N - 1]]).all()


def block_sum(terms, ok):
    """the fp64 sum of the definition: blocks of 128 positions, position ascending within, then block ascending"""
    total = np.zeros(terms.shape[1:])
    for g in range(0, len(terms), 128):
        acc = np.zeros(terms.shape[1:])
        for i in range(g, min(len(terms), g + 128)):
            if ok[i]:
                acc = acc + terms[i]
        total = total + acc
    return total


def test_ridge_loo_independent_of_the_twin(engine):
    """B = 0: e = t - tmean, so sse_fit is the block-ordered sum of its squares; dof is the block-ordered sum of lev0 + md2, md2 from
    Engine.index_project with scale S[l]"""
    N, dim, m, L, K = 700, 130, 40, 3, 2
    rows, t, mean, tmean, V, S, B, lev0 = head_ref.random_head(N, dim, m, L, K, seed=5)
    rows[100, 3] = np.nan
    t[200, 1] = np.nan
    ok = head_ref.counts(rows, t)
    ix = make_index(engine, rows)
    try:
        got = engine.index_ridge_loo(ix, t, mean, tmean, V, S, np.zeros_like(B), lev0)
        md2 = [engine.index_project(ix, mean, V, S[l])["md2"] for l in range(L)]
    finally:
        ix.free()
    d = (t - tmean).astype(np.float32).astype(np.float64)
    want = block_sum(d * d, ok)
    for l in range(L):
        pca_ref.same(got["sse_fit"][l], want, "sse_fit, strength %d" % l)
    lev = np.stack([(np.float32(lev0) + x).astype(np.float32) for x in md2], axis=1)
    pca_ref.same(got["dof"], block_sum(lev.astype(np.float64), ok), "dof")
    assert got["n"] == N - 2


def test_ridge_loo_over_two_chunks(engine, two_chunks):
    rows, ix = two_chunks
    N, dim, m, L, K = 17000, 1024, 3, 2, 1
    _, t, mean, tmean, V, S, B, lev0 = head_ref.random_head(64, dim, m, L, K, seed=6)
    t = targets_for(rows, 1, seed=3)
    t[16383, 0] = np.nan
    mean = rows[:100].mean(0).astype(np.float32)
    check_loo(engine, ix, [rows, t, mean, tmean, V, (S / 20).astype(np.float32), B, np.float32(1.0 / N)], np.array([1], np.int32), "two chunks")


def test_ridge_loo_of_an_empty_pool(engine):
    ix = engine.index_create(8)
    try:
        _, _, mean, tmean, V, S, B, lev0 = head_ref.random_head(4, 8, 2, 3, 2, seed=0)
        got = engine.index_ridge_loo(ix, np.zeros((0, 2), np.float32), mean, tmean, V, S, B, lev0)
        assert got["n"] == 0 and not got["sse"].any() and not got["dof"].any() and got["sse"].shape == (3, 2)
    finally:
        ix.free()


# ---- 3. the head behind a forward ----

def random_eval_head(dim, K, m, seed):
    rng = np.random.default_rng(seed)
    return dict(mean=rng.standard_normal(dim).astype(np.float32), tmean=rng.standard_normal(K).astype(np.float32),
                weights=(rng.standard_normal((K, dim)) / np.sqrt(dim)).astype(np.float32),
                components=(rng.standard_normal((m, dim)) / np.sqrt(dim)).astype(np.float32),
                scale=rng.uniform(0.01, 0.3, (K, m)).astype(np.float32), lev0=np.float32(0.01))


def check_head_batch(model, data, label):
    """head_batch == project_batch with (mean, W) and with (mean, V, S[k]) plus one fp32 add each; y and ga those of a plain forward"""
    from scann import _hip

    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(data))
    eng.forward_resident(rb)
    y, ga = eng.download(rb)
    for level in ("structure", "atom"):
        lvl = _hip.KNN_LEVELS[level]
        dim = model.config["model"]["dense_out" if level == "structure" else "global_dim"]
        K, m = 3, min(dim, 5)
        h = random_eval_head(dim, K, m, seed=dim + K)
        got = eng.head_batch(rb, lvl, h["mean"], h["tmean"], h["weights"], h["components"], h["scale"], h["lev0"])
        w = eng.project_batch(rb, lvl, h["mean"], h["weights"])
        pca_ref.same(got["pred"], (h["tmean"][None, :] + w["coords"]).astype(np.float32), "%s %s pred" % (label, level))
        for k in range(K):
            md2 = eng.project_batch(rb, lvl, h["mean"], h["components"], h["scale"][k])["md2"]
            pca_ref.same(np.ascontiguousarray(got["lev"][:, k]), (h["lev0"] + md2).astype(np.float32), "%s %s lev %d" % (label, level, k))
        pca_ref.same(got["y"], y, "y")
        pca_ref.same(got["ga"], ga, "ga")
    rb.free()


@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_head_batch_is_two_projections_and_an_add(hip_lib, kind):
    cfg, w, data, model = setup(kind=kind, n=24 if kind == "mp2018" else 40, seed=0)
    check_head_batch(model, data, kind)


def test_head_batch_on_a_generic_width_handle(hip_lib):
    """rows of 30 and 96 columns, the first no multiple of 4"""
    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    check_head_batch(model, data, "generic")


def child_scenario():
    cfg, w, data, model = setup(n=10, seed=3)
    check_head_batch(model, data, "child")
    return model.engine.exact_reruns()


def test_head_batch_on_an_exact_fp32_handle(hip_lib):
    """a handle whose forwards run exact-fp32 (SCANN_EXACT=1): a fresh process"""
    e = dict(os.environ)
    e["SCANN_EXACT"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 4. end to end ----

E2E = {"qm9": 64, "mp2018": 24}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_fit_head_is_the_host_route_on_the_models_rows(hip_lib, kind, level, tmp_path):
    from scann import _hip
    from scann.models import LatentHead

    n = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n, seed=0)
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    rows = index.rows()[0]
    t = targets_for(rows, 2, seed=4)
    t[3, 1] = np.nan
    got, head = model.fit_head(index, t, names=["a", "b"])
    want, head_w = head_ref.host_fit(rows, t, names=["a", "b"], level=level)
    pca_ref.same_moments(model.engine.index_fit_moments(index._ix, t), _hip.moments_host(head_ref.augmented(rows, t)), "%s %s" % (kind, level))
    print("%s %s: n_rows %d, l2 %s, loo_rmse %s, loo_r2 %s, dof %s" % (kind, level, got["n_rows"], got["l2"], got["loo_rmse"], got["loo_r2"], got["dof"]))
    assert sorted(got) == sorted(want) and got["n_rows"] == want["n_rows"] == len(rows) - 1 and got["names"] == ["a", "b"]
    for key in ("l2", "loo_rmse", "loo_mae", "loo_r2", "fit_rmse", "dof", "sigma2", "loo_prediction", "weights"):
        pca_ref.same(got[key], want[key], key)
    for key in ("l2", "loo_rmse", "dof"):
        pca_ref.same(got["path"][key], want["path"][key], "path " + key)
    for key in ("mean", "tmean", "weights", "components", "scale", "sigma2", "l2"):
        pca_ref.same(getattr(head, key), getattr(head_w, key), "head " + key)
    # predict_head right after, padded and packed: the head on the rows of the index, std at least sqrt(sigma2)
    a = model.predict_head(data, head, batch_size=16)
    pk = model.predict_head(_hip.pack_inputs(data), head, batch_size=16)
    y, _ = model.predict(data)
    assert np.array_equal(_bits(a["y"]), _bits(y)) and np.array_equal(_bits(pk["y"]), _bits(y))
    proj = _hip.project_host(rows, head.mean, head.weights) if head.k <= rows.shape[1] else None
    pca_ref.same(pk["prediction"], (head.tmean[None, :] + proj["coords"]).astype(np.float32), "prediction")
    assert pk["std"].shape == pk["prediction"].shape == (len(rows), 2) and np.all(pk["std"] >= np.sqrt(head.sigma2).astype(np.float32)[None, :])
    assert np.all(pk["leverage"] >= head.lev0)
    for key in ("prediction", "std", "leverage"):
        pca_ref.same(a[key], pk[key] if level == "structure" else _hip.repad_atoms(pk[key], data["atom_mask"], 0), "padded " + key)
    # data instead of an index (at atom level one array of targets per structure); save and load
    if level == "atom":
        counts = np.asarray(data["atom_mask"]).reshape(np.shape(data["neighbors"])[:2]).astype(bool).sum(1)
        per = np.split(t, np.cumsum(counts)[:-1])
        direct, _ = model.fit_head(data, per, level="atom", batch_size=16, names=["a", "b"])
    else:
        direct, _ = model.fit_head(data, t, batch_size=16, names=["a", "b"])
    pca_ref.same(direct["loo_prediction"], got["loo_prediction"], "direct")
    head.save(str(tmp_path / "head.npz"))
    back = LatentHead.load(model, str(tmp_path / "head.npz"))
    pca_ref.same(model.predict_head(data, back, batch_size=16)["std"], a["std"], "loaded head")
    index.free()


# ---- 5. state ----

def test_nothing_else_changes(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool, rb, rows = u.eng, u.pool, u.rb, u.rows[0]
        t = targets_for(rows, 2, seed=7)
        _, _, _, _, V, S, B, lev0 = head_ref.random_head(8, 128, 6, 4, 2, seed=7)
        mean, tmean = rows.mean(0).astype(np.float32), t.mean(0).astype(np.float32)
        first_m = eng.index_fit_moments(pool, t)
        first_l = eng.index_ridge_loo(pool, t, mean, tmean, V, S, B, lev0, np.array([1, 3], np.int32))

        def same(r):
            pca_ref.same_moments(r[0], first_m, "repeat")
            head_ref.same_loo(r[1], first_l, "repeat")

        u.repeat(lambda: (eng.index_fit_moments(pool, t), eng.index_ridge_loo(pool, t, mean, tmean, V, S, B, lev0, np.array([1, 3], np.int32))),
                 same, 5, 16 << 20)
        u.check()
        # head_batch: y is the plain forward's; the selection is put back
        h = random_eval_head(128, 2, 4, seed=1)
        r = eng.head_batch(rb, _hip.OUT_BF_PROPERTY, h["mean"], h["tmean"], h["weights"], h["components"], h["scale"], h["lev0"])
        assert np.array_equal(_bits(r["y"]), _bits(u.y_first))
        u.reforward()


def test_training_handle(hip_lib):
    """after two training steps the calls on the training handle equal the host twins', and weights, gradients and the following
    (deterministic) step -- the Adam state entered it -- are those of a twin that never made the calls"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    args = list(head_ref.random_head(900, 128, 20, 4, 2, seed=8))
    h = random_eval_head(128, 2, 4, seed=2)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, args[0])
        pca_ref.same_moments(eng.index_fit_moments(ix, args[1]), _hip.moments_host(head_ref.augmented(args[0], args[1])), "training handle")
        check_loo(eng, ix, args, np.array([0, 3], np.int32), "training handle")
        ix.free()
        inf_model, rb2 = inference()
        inf = inf_model.engine
        for level in (_hip.OUT_BF_PROPERTY, _hip.OUT_AFTER_LC):
            hb = [e.head_batch(b, level, h["mean"], h["tmean"], h["weights"], h["components"], h["scale"], h["lev0"]) for e, b in ((eng, rb), (inf, rb2))]
            for key in hb[0]:
                pca_ref.same(hb[0][key], hb[1][key], "training against inference handle, " + key)

    training_twin(cfg, w, pk, calls)


# ---- 6. errors, the CLI ----

def test_errors_name_what_is_wrong(hip_lib):
    import ctypes as C

    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows, t, mean, tmean, V, S, B, lev0 = head_ref.random_head(5, 4, 2, 2, 2, seed=0)
    pool, foreign, empty = make_index(eng, rows), make_index(other.engine, rows), eng.index_create(4)
    P = _hip._ptr
    out = {"sse": np.full((2, 2), 7.0), "mean": np.full(6, 7, np.float32), "cov": np.full((6, 6), 7.0), "resid": np.full((5, 2), 7, np.float32)}
    q = [np.zeros((2, 2)), np.zeros((2, 2)), np.zeros(2)]
    n = C.c_int64(-5)

    def moments(p=pool, t=t, K=2, n=n, mean=out["mean"], cov=out["cov"]):
        return eng.lib.scann_index_fit_moments(eng._h, None if p is None else p._h, P(t), K, None if n is None else C.byref(n), P(mean), P(cov), None, None)

    def loo(p=pool, t=t, K=2, mean=mean, tmean=tmean, V=V, m=2, S=S, B=B, L=2, lev0=float(lev0), rl=None, n=n, sse=out["sse"], resid=None):
        return eng.lib.scann_index_ridge_loo(eng._h, None if p is None else p._h, P(t), K, P(mean), P(tmean), P(V), m, P(S), P(B), L, lev0, P(rl),
                                             None if n is None else C.byref(n), P(sse), P(q[0]), P(q[1]), P(q[2]), P(resid))

    def message(e=eng):
        return (eng.lib.scann_last_error(e._h) or b"").decode()

    def with_nan(a, at):
        b = a.copy()
        b.reshape(-1)[at] = np.nan
        return b

    free0, _ = eng.device_memory()
    assert moments(p=None) == -1 and "null" in message()
    assert moments(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert moments(K=0) == -1 and "K 0 outside 1 .. 16" in message()
    assert moments(K=17) == -1 and "K 17 outside 1 .. 16" in message()
    assert moments(t=None) == -1 and "targets is null" in message()
    assert moments(n=None) == -1 and "n_eligible is null" in message()
    assert moments(mean=None) == -1 and "mean is null" in message()
    assert moments(cov=None) == -1 and "cov is null" in message()
    assert moments(p=empty) == -1 and "at least 2 rows" in message() and "has 0" in message()
    few = t.copy()
    few[1:] = np.nan
    assert moments(t=few) == -1 and "has 1 among its 5" in message() and n.value == 1
    assert loo(p=None) == -1 and "null" in message()
    assert loo(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert loo(K=17) == -1 and "K 17 outside 1 .. 16" in message()
    assert loo(L=0) == -1 and "L 0 outside 1 .. 32" in message()
    assert loo(L=33) == -1 and "L 33 outside 1 .. 32" in message()
    assert loo(m=0) == -1 and "m 0 outside 1 .. 4" in message()
    assert loo(m=5) == -1 and "m 5 outside 1 .. 4" in message()
    for kw, word in ((dict(t=None), "targets is null"), (dict(mean=None), "mean is null"), (dict(tmean=None), "tmean is null"),
                     (dict(V=None), "components is null"), (dict(S=None), "scale is null"), (dict(B=None), "coef is null"),
                     (dict(n=None), "n_used is null"), (dict(sse=None), "sse is null"), (dict(rl=np.zeros(2, np.int32)), "resid_l needs resid"),
                     (dict(mean=with_nan(mean, 2)), "mean holds a non-finite value (column 2)"),
                     (dict(tmean=with_nan(tmean, 1)), "tmean holds a non-finite value (target 1)"),
                     (dict(V=with_nan(V, 5)), "components hold a non-finite value (component 1)"),
                     (dict(S=with_nan(S, 3)), "scale holds a non-finite value (strength 1)"),
                     (dict(B=with_nan(B, 4)), "coef holds a non-finite value (strength 1)"), (dict(lev0=float("inf")), "lev0 is not finite"),
                     (dict(rl=np.array([0, 2], np.int32), resid=out["resid"]), "resid_l[1] = 2 outside -1 .. 1"),
                     (dict(rl=np.array([-2, 0], np.int32), resid=out["resid"]), "resid_l[0] = -2 outside -1 .. 1")):
        assert loo(**kw) == -1 and word in message(), (word, message())
    rb = eng.upload(_hip.pack_inputs(data))
    h = random_eval_head(128, 2, 3, seed=0)
    pred = np.full((4, 2), 7, np.float32)

    def batch(level=_hip.OUT_BF_PROPERTY, b=rb, K=2, m=3, pred=pred, **kw):
        a = dict(h)
        a.update(kw)
        return eng.lib.scann_head_batch(eng._h, None if b is None else b._h, level, P(a["mean"]), P(a["tmean"]), P(a["weights"]), K, P(a["components"]), m,
                                        P(a["scale"]), float(a["lev0"]), None, None, P(pred), P(np.zeros((4, 2), np.float32)))

    assert batch(b=None) == -1 and "null handle or batch" in message()
    assert batch(level=9) == -1 and "level must be" in message() and "got 9" in message()
    assert batch(K=17) == -1 and "K 17 outside 1 .. 16" in message()
    assert batch(m=129) == -1 and "m 129 outside 1 .. 128" in message()
    assert batch(weights=None) == -1 and "weights is null" in message()
    assert batch(pred=None) == -1 and "pred is null" in message()
    assert batch(weights=with_nan(h["weights"], 130)) == -1 and "weights hold a non-finite value (target 1)" in message()
    assert batch(scale=with_nan(h["scale"], 0)) == -1 and "scale holds a non-finite value (target 0)" in message()
    assert batch(lev0=np.nan) == -1 and "lev0 is not finite" in message()
    # nothing was written, nothing stays allocated
    assert np.all(out["sse"] == 7) and np.all(out["mean"] == 7) and np.all(out["cov"] == 7) and np.all(out["resid"] == 7) and np.all(pred == 7)
    assert free0 - eng.device_memory()[0] <= 8 << 20
    assert moments() == 0 and n.value == 5 and loo() == 0 and n.value == 5 and batch() == 0
    rb.free()
    # the Python layers: ValueError before any device call
    lat = model.build_index(data)
    for bad in (np.zeros(3), np.zeros((4, 17)), "x"):
        with pytest.raises(ValueError):
            lat.fit_head(bad)
    with pytest.raises(ValueError):
        lat.fit_head(np.zeros(4), l2="cv")
    with pytest.raises(ValueError, match="at least 3 rows"):
        lat.fit_head(np.float32([1, 2, np.nan, np.nan]))
    with pytest.raises(ValueError):
        other.fit_head(lat, np.zeros(4))  # another model's index
    with pytest.raises(ValueError):
        model.predict_head(data, "a head")
    for ix in (pool, foreign, empty, lat):
        ix.free()


def test_cli_fits_and_applies_a_head(hip_lib, tmp_path):
    """predict_model.py --fit-head writes head_<target>.pickle and, with --head-out, the head; --head applies it; the other files' bytes
    are those of a run without the flags"""
    import yaml

    from scann.models import SCANN, LatentHead
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
    r = subprocess.run(cli + ["--fit-head", str(tmp_path / "t.npy"), "--head-out", str(tmp_path / "head.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"head_homo.pickle"}
    got = pickle.load(open(out / "head_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="structure", ids=data.indexes)
    want, head = scann.fit_head(pool, t)
    assert sorted(got) == sorted(list(want) + ["id", "atom"])
    for key in ("l2", "loo_rmse", "loo_r2", "loo_prediction", "weights"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert "loo_rmse" in r.stdout and "target_1" in r.stdout and "n_rows %d" % n in r.stdout
    saved = LatentHead.load(scann.model, str(tmp_path / "head.npz"))
    for key in ("mean", "tmean", "weights", "components", "scale", "sigma2"):
        pca_ref.same(getattr(saved, key), getattr(head, key), key)
    r = subprocess.run(cli + ["--head", str(tmp_path / "head.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    per = pickle.load(open(out / "head_homo.pickle", "rb"))
    assert len(per) == n and sorted(per[0]) == ["leverage", "predict_property", "prediction", "std"] and per[0]["prediction"].shape == (2,)
    inputs, _ = data[0]
    first = scann.predict_head(inputs, head)
    assert np.array_equal(per[0]["prediction"], first["prediction"][0]) and np.array_equal(per[0]["std"], first["std"][0])
    pool.free()


if __name__ == "__main__":
    reruns = child_scenario()
    print("child ok, exact re-runs %d" % reruns)

"""GPU tests of the principal-component map (scann_index_moments / scann_index_project / scann_project_batch through Engine.index_moments,
index_project, project_batch; LatentIndex.pca, HipModel.fit_projection / project).  Every comparison of a device result is an equality
of bit patterns (a NaN equals a NaN).

1. Engine.index_moments == the host twin (scann_moments_host): N either side of the 32-row slab and of the 128-row tile; dim 1, below a
   64-column block, off the multiple of 32, the maximum; a pool of two storage chunks, where b drops to 23, against the NumPy
   restatement on 16 rows of the matrix; planted NaN / inf rows and a constant column; one add or many, unrelated indices in between.
2. Engine.index_project == the twin (scann_project_host) at the same edges, m ragged against the block of 64 components; independent of
   the twin: dist2 == Engine.index_query (k = 1) against an index that holds only the mean.
3. End to end on the qm9 and mp2018 fixtures at both levels.  4. Non-interference.  5. Errors name what is wrong.  6. The CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import pca_ref
import scann_oracle as so
from analysis_checks import SUBNORMAL, _bits, make_index, random_rows, scan_edge_rows, setup, training_twin, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def random_projection(dim, m, seed=0):
    rng = np.random.default_rng(dim * 11 + m + seed)
    return (rng.standard_normal(dim).astype(np.float32), rng.standard_normal((m, dim)).astype(np.float32),
            rng.uniform(0.1, 2, m).astype(np.float32))


# (N, dim).  A slab of the scatter kernel is 32 rows, a tile of the projection 128, a column block 64 columns, a slab 32 columns
SHAPES = [(2, 3), (31, 1), (32, 16), (33, 16), (127, 128), (128, 128), (129, 130), (1000, 3), (5000, 130), (600, 1024)]


@pytest.fixture(scope="module")
def two_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns"""
    rows = random_rows(17000, 1024)
    ix = make_index(engine, rows)
    yield rows, ix
    ix.free()


@pytest.mark.parametrize("N,dim", SHAPES, ids=["N%d_d%d" % c for c in SHAPES])
def test_moments_equal_the_host_twin(engine, N, dim):
    from scann import _hip

    rows = random_rows(N, dim)
    want = _hip.moments_host(rows)
    ix = make_index(engine, rows)
    try:
        got = engine.index_moments(ix)
        again = engine.index_moments(ix)
    finally:
        ix.free()
    print("N %d dim %d: n %d bits %d, %d cov values differ" % (N, dim, got["n"], got["bits"], int((got["cov"].view(np.uint64) != want["cov"].view(np.uint64)).sum())))
    pca_ref.same_moments(got, want, "N %d dim %d" % (N, dim))
    pca_ref.same_moments(again, got, "repeat")
    assert np.array_equal(got["cov"], got["cov"].T) and got["bits"] == 24


def test_moments_over_two_chunks(engine, two_chunks):
    rows, ix = two_chunks
    got = engine.index_moments(ix)
    only = list(range(8)) + list(range(1016, 1024))
    want = pca_ref.moments(rows, only=only)
    assert got["n"] == 17000 and got["bits"] == 23
    pca_ref.same(got["mean"], want["mean"], "mean")
    pca_ref.same(got["col_exp"], want["col_exp"], "col_exp")
    pca_ref.same(got["cov"][only], want["cov"], "cov rows")
    assert np.array_equal(got["cov"], got["cov"].T)


def test_moments_of_planted_rows(engine):
    from scann import _hip

    rows = random_rows(700, 130, seed=12)
    rows[13, 129] = np.nan
    rows[300, 128] = np.inf
    rows[699, 0] = -np.inf
    rows[:, 7] = 2.5  # a constant column: its variance is exactly 0
    ix = make_index(engine, rows)
    try:
        got = engine.index_moments(ix)
    finally:
        ix.free()
    pca_ref.same_moments(got, _hip.moments_host(rows), "planted")
    pca_ref.same_moments(got, pca_ref.moments(rows), "planted, NumPy")
    assert got["n"] == 697 and not got["cov"][7].any() and not got["cov"][:, 7].any() and got["mean"][7] == 2.5
    # all rows equal: the covariance is exactly 0
    same_rows = np.tile(random_rows(1, 16, seed=3), (50, 1))
    ix = make_index(engine, same_rows)
    try:
        got = engine.index_moments(ix)
    finally:
        ix.free()
    assert not got["cov"].any() and np.array_equal(_bits(got["mean"]), _bits(same_rows[0]))


def test_moments_at_the_edges_of_the_eligibility_scan(engine):
    """n says which rows the scan found eligible; mean and col_exp of the subnormal column carry frexp's exponent of its maximum"""
    from scann import _hip

    for label, rows in scan_edge_rows():
        ix = make_index(engine, rows)
        try:
            if len(rows) < 2:  # a covariance needs two rows: the twin refuses the index, and the device does once its scan has counted the one
                with pytest.raises(ValueError, match="at least 2 rows"):
                    _hip.moments_host(rows)
                with pytest.raises(_hip.ScannHipError, match="has 1 among its 1"):
                    engine.index_moments(ix)
                continue
            got = engine.index_moments(ix)
        finally:
            ix.free()
        pca_ref.same_moments(got, _hip.moments_host(rows), label)
        assert got["n"] == np.isfinite(rows).all(axis=1).sum(), label
        if rows.shape[1] >= 5:
            assert 0 < got["mean"][1] < 400 * SUBNORMAL and got["col_exp"][1] < -125, label


def test_moments_do_not_depend_on_how_the_index_was_built(engine):
    rng = np.random.default_rng(9)
    dim, N = 130, 3000
    rows = random_rows(N, dim, seed=9)
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
        a = engine.index_moments(one)
        for d in (64, 130, 7):  # unrelated indices come and go in between (workspace and chunks share one block cache)
            tmp = make_index(engine, rng.standard_normal((900, d)).astype(np.float32))
            engine.index_moments(tmp)
            tmp.free()
        for ix in (many, one):
            pca_ref.same_moments(engine.index_moments(ix), a, "many adds")
        # a permutation of the rows: the same bits
        perm = make_index(engine, rows[rng.permutation(N)])
        try:
            pca_ref.same_moments(engine.index_moments(perm), a, "permuted")
        finally:
            perm.free()
    finally:
        one.free()
        many.free()


def check_projection(eng, ix, rows, m, label, with_scale=True):
    from scann import _hip

    mean, comp, scale = random_projection(rows.shape[1], m)
    scale = scale if with_scale else None
    got = eng.index_project(ix, mean, comp, scale)
    want = _hip.project_host(rows, mean, comp, scale)
    print("%s: N %d dim %d m %d: %d coordinates differ" % (label, len(rows), rows.shape[1], m, int((_bits(got["coords"]) != _bits(want["coords"])).sum())))
    pca_ref.same_projection(got, want, "%s m %d" % (label, m))
    return mean, got


@pytest.mark.parametrize("N,dim", SHAPES, ids=["N%d_d%d" % c for c in SHAPES])
def test_projection_equals_the_host_twin(engine, N, dim):
    rows = random_rows(N, dim)
    if N >= 100:
        rows[5, dim - 1] = np.nan  # a NaN propagates; no eligibility pass
        rows[6, 0] = np.inf
    ix = make_index(engine, rows)
    try:
        for m in sorted({m for m in (1, 2, 63, 64, 65, dim) if m <= dim}):
            mean, got = check_projection(engine, ix, rows, m, "random")
        check_projection(engine, ix, rows, 1, "no scale", with_scale=False)
        # a part of the rows, from a position that is no multiple of anything
        if N > 40:
            mean3, comp, scale = random_projection(dim, min(dim, 3))
            part = engine.index_project(ix, mean3, comp, scale, first=37, n=N - 40)
            whole = engine.index_project(ix, mean3, comp, scale)
            pca_ref.same_projection(part, {k: v[37:N - 3] for k, v in whole.items()}, "part")
        # independent of the twin: dist2 is the k = 1 query against an index that holds only the mean (a NaN distance never qualifies
        # there: the rows with a non-finite component are left out)
        mix = make_index(engine, mean[None, :])
        try:
            q = engine.index_query(mix, rows, 1)
        finally:
            mix.free()
        ok = np.isfinite(rows).all(axis=1)
        pca_ref.same(got["dist2"][ok], q["dist2"][ok, 0], "dist2 against the query")
    finally:
        ix.free()


@pytest.mark.parametrize("dim", [1, 3, 130])
def test_projection_does_not_walk_the_padding(engine, dim):
    """a chain ends at column dim - 1: products that underflow to -0 leave a coordinate of -0.0, as in the twin; walking the zero
    padding up to the stored width with fmaf(0, 0, acc) would make it +0.0"""
    from scann import _hip

    rows = np.full((5, dim), 1e-30, np.float32)
    mean, comp = np.zeros(dim, np.float32), np.full((1, dim), -1e-30, np.float32)
    want = _hip.project_host(rows, mean, comp)
    assert np.all(_bits(want["coords"]) == 0x80000000)
    ix = make_index(engine, rows)
    try:
        pca_ref.same_projection(engine.index_project(ix, mean, comp), want, "negative zero, dim %d" % dim)
    finally:
        ix.free()


def test_projection_over_two_chunks(engine, two_chunks):
    rows, ix = two_chunks
    check_projection(engine, ix, rows, 3, "two chunks")


# ---- end to end ----

E2E = {"qm9": 64, "mp2018": 24}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_fit_projection_is_the_host_map_of_the_models_rows(hip_lib, kind, level, tmp_path):
    from scann import _hip
    from scann.models import LatentProjection

    n = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n, seed=0)
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    rows = index.rows()[0]
    m = 3
    got, proj = model.fit_projection(index, m=m)
    mo = _hip.moments_host(rows)
    pca_ref.same_moments(model.engine.index_moments(index._ix), mo, "%s %s" % (kind, level))
    wv, v, sweeps = _hip.sym_eig(mo["cov"])
    noise = rows.shape[1] * 2.0 ** (2 * int(mo["col_exp"].max()) - mo["bits"] + 2)
    comp = v[:m].astype(np.float32)
    scale = np.where(wv[:m] > noise, 1 / np.sqrt(np.where(wv[:m] > noise, wv[:m], 1)), 0).astype(np.float32)
    want = _hip.project_host(rows, mo["mean"], comp, scale)
    pca_ref.same(got["mean"], mo["mean"], "mean")
    pca_ref.same(got["components"], comp, "components")
    pca_ref.same(got["variance"], wv[:m], "variance")
    pca_ref.same(proj.scale, scale, "scale")
    pca_ref.same(got["coordinates"], want["coords"], "coordinates")
    pca_ref.same(got["mahalanobis"], np.sqrt(want["md2"]), "mahalanobis")
    pca_ref.same(got["distance_to_mean"], np.sqrt(want["dist2"]), "distance_to_mean")
    assert got["n_rows"] == len(rows) and got["rank"] == int((wv > noise).sum()) and got["noise_floor"] == noise
    assert got["total_variance"] == float(np.trace(mo["cov"]))
    full, _ = index.pca()
    for name, r in (("m = 3", got), ("m = dim", full)):
        ratio = r["explained_variance_ratio"]
        print("%s %s, %s: rank %d of %d, sweeps %d, ratio[:3] %s, sum %.17g" % (kind, level, name, r["rank"], rows.shape[1], sweeps, ratio[:3], ratio.sum()))
        assert ratio.dtype == np.float64 and np.all(ratio >= 0) and np.all(np.diff(ratio) <= 0)
        assert ratio.sum() <= 1 and float(np.cumsum(ratio)[-1]) <= 1 and float(np.cumsum(ratio[::-1])[-1]) <= 1
    pca_ref.same(got["explained_variance_ratio"], full["explained_variance_ratio"][:m], "the leading ratios of the full map")
    assert abs(full["explained_variance_ratio"].sum() - 1) <= 4 * rows.shape[1] * 2.0 ** -52  # (the divisor's margin, and no more)
    pca_ref.same(full["coordinates"][:, :m], got["coordinates"], "the leading coordinates of the full map")
    # project on the same inputs reproduces the coordinates, padded and packed
    a = model.project(data, proj, batch_size=16)
    pk = model.project(_hip.pack_inputs(data), proj, batch_size=16)
    y, _ = model.predict(data)
    assert np.array_equal(_bits(a["predict_property"]), _bits(y)) and np.array_equal(_bits(pk["predict_property"]), _bits(y))
    for key in ("coordinates", "mahalanobis", "distance_to_mean"):
        pca_ref.same(pk[key], got[key], "packed " + key)
        pca_ref.same(a[key], got[key] if level == "structure" else _hip.repad_atoms(got[key], data["atom_mask"], 0), "padded " + key)
    # data instead of an index: indexed for the call and freed; the same map.  Save and load: the same projection
    direct, p2 = model.fit_projection(data, m=m, level=level, batch_size=16)
    pca_ref.same(direct["coordinates"], got["coordinates"], "direct")
    proj.save(str(tmp_path / "map.npz"))
    back = LatentProjection.load(model, str(tmp_path / "map.npz"))
    for key in ("mean", "components", "variance", "scale"):
        pca_ref.same(getattr(back, key), getattr(proj, key), "loaded " + key)
    assert back.level == level and back.rank == proj.rank and back.noise_floor == proj.noise_floor
    index.free()


# ---- state, errors ----

def test_nothing_else_changes(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=40, seed=2)
    mean, comp, scale = random_projection(128, 5)
    with untouched(model, data) as u:
        eng, pool, rb = u.eng, u.pool, u.rb
        first = eng.index_moments(pool)
        first_p = eng.index_project(pool, mean, comp, scale)

        def same(r):
            pca_ref.same_moments(r[0], first, "repeat")
            pca_ref.same_projection(r[1], first_p, "repeat")

        u.repeat(lambda: (eng.index_moments(pool), eng.index_project(pool, mean, comp, scale)), same, 10, 16 << 20)
        u.check()
        # project_batch: y and ga are those of a plain forward, the rows those of the pool; the selection is put back
        r = eng.project_batch(rb, _hip.OUT_AFTER_LC, mean, comp, scale)
        assert np.array_equal(_bits(r["y"]), _bits(u.y_first))
        pca_ref.same_projection({k: r[k] for k in first_p}, first_p, "project_batch")
        u.reforward()


def test_device_memory_after_free(hip_lib):
    """an index that is freed gives its chunks back, and so does the temporary index of fit_projection(data): after a first round that
    fills the block cache, eight more rounds of create / moments / project / free take nothing further from the device.  (A chunk is
    64 MiB: one that leaked per round would be 512 MiB.)"""
    cfg, w, data, model = setup(n=40, seed=2)
    eng = model.engine
    rows = random_rows(3000, 128)
    mean, comp, scale = random_projection(128, 5)

    def one_round():
        ix = make_index(eng, rows)
        eng.index_moments(ix)
        eng.index_project(ix, mean, comp, scale)
        ix.free()
        result, proj = model.fit_projection(data, m=2, level="atom", batch_size=16)
        return result

    first = one_round()
    free0, _ = eng.device_memory()
    for rep in range(8):
        pca_ref.same(one_round()["coordinates"], first["coordinates"], "round %d" % rep)
    free1, _ = eng.device_memory()
    print("device memory free before / after eight rounds: %d / %d" % (free0, free1))
    assert free0 - free1 <= 16 << 20, (free0, free1)


def test_training_handle(hip_lib):
    """after two training steps the moments and a projection on the training handle equal the host twins', and weights, gradients and
    the following (deterministic) step are those of a twin that never made the calls"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows = random_rows(900, 128)
    mean, comp, scale = random_projection(128, 4)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, rows)
        pca_ref.same_moments(eng.index_moments(ix), _hip.moments_host(rows), "training handle")
        pca_ref.same_projection(eng.index_project(ix, mean, comp, scale), _hip.project_host(rows, mean, comp, scale), "training handle")
        ix.free()
        # project_batch: what an inference handle with the same weights gives, y and ga those of its forward + download, and the
        # projection of the level's rows as add_batch stores them
        inf_model, rb2 = inference()
        inf = inf_model.engine
        inf.forward_resident(rb2)
        y_inf, ga_inf = inf.download(rb2)
        for level in (_hip.OUT_BF_PROPERTY, _hip.OUT_AFTER_LC):
            r, r_inf = eng.project_batch(rb, level, mean, comp, scale), inf.project_batch(rb2, level, mean, comp, scale)
            for key in r:
                pca_ref.same(r[key], r_inf[key], "training against inference handle, " + key)
            pca_ref.same(r["y"], y_inf, "y")
            pca_ref.same(r["ga"], ga_inf, "ga")
            tmp = eng.index_create(128)
            eng.index_add_batch(tmp, rb, level)
            level_rows = eng.index_read(tmp)[0]
            tmp.free()
            assert len(level_rows) == (pk.n_atom if level == _hip.OUT_AFTER_LC else pk.n_struct)
            pca_ref.same_projection({k: r[k] for k in ("coords", "md2", "dist2")}, _hip.project_host(level_rows, mean, comp, scale), "project_batch")

    training_twin(cfg, w, pk, calls)


def test_generic_width_handle(hip_lib):
    """a handle of widths other than 128 / 8: rows of 30 and 96 columns, the first no multiple of 4"""
    from scann import _hip

    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    for level in ("structure", "atom"):
        ix = model.build_index(data, level=level, batch_size=4)
        rows = ix.rows()[0]
        got, proj = ix.pca(2)
        mo = _hip.moments_host(rows)
        pca_ref.same(got["mean"], mo["mean"], "mean")
        want = _hip.project_host(rows, proj.mean, proj.components, proj.scale)
        pca_ref.same(got["coordinates"], want["coords"], "coordinates")
        a = model.project(_hip.pack_inputs(data), proj, batch_size=4)
        pca_ref.same(a["coordinates"], got["coordinates"], "project")
        pca_ref.same(a["mahalanobis"], got["mahalanobis"], "mahalanobis")
        ix.free()


def test_errors_name_what_is_wrong(hip_lib):
    import ctypes as C

    from scann import _hip
    from scann.models import LatentProjection

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows = np.arange(12, dtype=np.float32).reshape(3, 4) ** 2
    rows_bad = rows.copy()
    rows_bad[1, 2] = np.nan
    rows_bad[2, 0] = np.inf
    pool, dirty, foreign, empty = make_index(eng, rows), make_index(eng, rows_bad), make_index(other.engine, rows), eng.index_create(4)
    single, single_bad = make_index(eng, rows[:1]), make_index(eng, rows_bad[1:2])  # one row: n_eligible says whether it counts
    P = _hip._ptr
    out = {"mean": np.full(4, 7, np.float32), "cov": np.full((4, 4), 7, np.float64), "coords": np.full((3, 2), 7, np.float32)}
    ne = C.c_int64(-5)
    mean, comp, scale = random_projection(4, 2)

    def moments(p=pool, n=ne, mean=out["mean"], cov=out["cov"], handle=eng):
        return eng.lib.scann_index_moments(handle._h, None if p is None else p._h, None if n is None else C.byref(n), P(mean), P(cov), None, None)

    def project(p=pool, first=0, n=3, mean=mean, comp=comp, scale=scale, m=2, coords=out["coords"], md2=None, handle=eng):
        return eng.lib.scann_index_project(handle._h, None if p is None else p._h, first, n, P(mean), P(comp), P(scale), m, P(coords), P(md2), None)

    def message(e=eng):
        return (eng.lib.scann_last_error(e._h) or b"").decode()

    def with_nan(a, at):
        b = a.copy()
        b.reshape(-1)[at] = np.nan
        return b

    free0, _ = eng.device_memory()
    assert moments(p=None) == -1 and "null" in message()
    assert moments(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert moments(handle=other.engine) == -1 and "another handle" in message(other.engine)
    assert moments(n=None) == -1 and "n_eligible is null" in message()
    assert moments(mean=None) == -1 and "mean is null" in message()
    assert moments(cov=None) == -1 and "cov is null" in message()
    assert moments(p=empty) == -1 and "at least 2 rows" in message() and "has 0" in message()
    assert moments(p=dirty) == -1 and "at least 2 rows" in message() and "has 1 among its 3" in message() and ne.value == 1
    assert moments(p=single) == -1 and "has 1 among its 1" in message() and ne.value == 1
    assert moments(p=single_bad) == -1 and "has 0 among its 1" in message() and ne.value == 0
    assert project(p=None) == -1 and "null" in message()
    assert project(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert project(first=2, n=2) == -1 and "rows 2 .. 4 of 3" in message()
    assert project(first=-1) == -1 and "rows -1" in message()
    assert project(m=0) == -1 and "m 0 outside 1 .. 4" in message()
    assert project(m=5) == -1 and "m 5 outside 1 .. 4" in message()
    assert project(mean=None) == -1 and "mean is null" in message()
    assert project(comp=None) == -1 and "components is null" in message()
    assert project(coords=None) == -1 and "coords is null" in message()
    assert project(scale=None, md2=np.zeros(3, np.float32)) == -1 and "scale" in message() and "null" in message()
    assert project(mean=with_nan(mean, 2)) == -1 and "mean holds a non-finite value (column 2)" in message()
    assert project(comp=with_nan(comp, 5)) == -1 and "components hold a non-finite value (component 1, column 1)" in message()
    assert project(scale=with_nan(scale, 1)) == -1 and "scale holds a non-finite value (component 1)" in message()
    rb = eng.upload(_hip.pack_inputs(data))
    m128 = random_projection(128, 2)

    def batch(level=_hip.OUT_BF_PROPERTY, mean=m128[0], comp=m128[1], m=2, coords=np.zeros((4, 2), np.float32), b=rb):
        return eng.lib.scann_project_batch(eng._h, None if b is None else b._h, level, P(mean), P(comp), None, m, None, None, P(coords), None, None)

    assert batch(b=None) == -1 and "null handle or batch" in message()
    assert batch(level=9) == -1 and "level must be" in message() and "got 9" in message()
    assert batch(m=129) == -1 and "m 129 outside 1 .. 128" in message()
    assert batch(mean=with_nan(m128[0], 3)) == -1 and "mean holds a non-finite value (column 3)" in message()
    assert batch(coords=None) == -1 and "coords is null" in message()
    # nothing was written, nothing stays allocated
    assert np.all(out["mean"] == 7) and np.all(out["cov"] == 7) and np.all(out["coords"] == 7)
    assert free0 - eng.device_memory()[0] <= 8 << 20
    assert moments() == 0 and ne.value == 3 and project() == 0 and batch() == 0
    rb.free()
    # the Python layers: ValueError before any device call
    for kw in (dict(mean=mean[:3]), dict(components=comp[:, :3]), dict(components=np.zeros((5, 4), np.float32)), dict(scale=scale[:1]),
               dict(mean=with_nan(mean, 0)), dict(components=with_nan(comp, 0)), dict(scale=with_nan(scale, 0)), dict(first=2, n=2), dict(mean="x")):
        args = dict(mean=mean, components=comp, scale=scale)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.index_project(pool, **args)
    lat = model.build_index(data)
    for m in (0, 129, 2.5, True, "2"):
        with pytest.raises(ValueError):
            lat.pca(m)
        with pytest.raises(ValueError):
            model.fit_projection(data, m=m)
    one = model.build_index({k: v[:1] for k, v in data.items()})
    with pytest.raises(ValueError, match="at least 2 rows"):
        one.pca(1)
    result, proj = lat.pca(2)
    with pytest.raises(ValueError):
        model.fit_projection(data, level="bond")
    with pytest.raises(ValueError):
        model.fit_projection(data, batch_size=0)
    with pytest.raises(ValueError):
        other.fit_projection(lat)  # another model's index
    with pytest.raises(ValueError):
        model.project(data, "a projection")
    with pytest.raises(ValueError):
        model.project(data, LatentProjection(np.zeros(64, np.float32), np.ones((2, 64), np.float32), [2.0, 1.0], 0.0, "structure"))
    with pytest.raises(ValueError):
        model.project(data, proj, batch_size=0)
    with pytest.raises(ValueError):
        model.build_index(data, level="atom").project(proj)  # a structure-level projection
    for ix in (pool, dirty, foreign, empty, single, single_bad, lat, one):
        ix.free()


def test_cli_writes_the_projection(hip_lib, tmp_path):
    """predict_model.py --project 2: projection_<target>.pickle and, with --project-out, the map; the other files' bytes are those of a
    run without the flag"""
    import yaml

    from scann.models import SCANN, LatentProjection
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
    r = subprocess.run(cli + ["--project", "2", "--project-level", "atom", "--project-out", str(tmp_path / "map.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"projection_homo.pickle"}
    got = pickle.load(open(out / "projection_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    want, proj = scann.fit_projection(pool, m=2)
    assert sorted(got) == sorted(list(want) + ["id", "atom"])
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    ids, atoms = scann.model.engine.index_names(pool._ix)
    assert np.array_equal(got["id"], ids) and np.array_equal(got["atom"], atoms)
    assert "rank %d" % want["rank"] in r.stdout and "n_rows %d" % len(pool) in r.stdout
    saved = LatentProjection.load(scann.model, str(tmp_path / "map.npz"))
    assert saved.level == "atom"
    for key in ("mean", "components", "variance", "scale"):
        pca_ref.same(getattr(saved, key), getattr(proj, key), key)
    pool.free()

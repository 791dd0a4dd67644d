"""GPU tests of the density-peak clustering and the kernel density of a latent index (scann_index_density / scann_index_peaks /
scann_index_density_batch through Engine.index_density, index_peaks, density_batch; LatentIndex.density_peaks, HipModel.density_peaks /
density).  Every comparison of a device result with a twin is an equality: integers equal, floats bit for bit.

1. The kernels == the twins scann_density_host / scann_peaks_host: N either side of the 64-row tile and of the 128-query tile, one and
   many workgroups, dim either side of the 32-column slab and no multiple of 4, the smallest and the largest widths; planted ties,
   coincident rows, non-finite rows, distances that overflow; skipped positions.  2. Two storage chunks.  3. One add or many; after
   unrelated indices were created and freed.  4. End to end on the qm9 and mp2018 fixtures at both levels, with the reference's
   certificate; the density behind a forward; a generic width; a training handle.  5. Non-interference.  6. Errors; the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import peaks_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import _bits, make_index, random_rows, same_arrays, setup, training_twin, untouched  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def gamma_for(rows, u=6.0):
    """a gamma that spreads u = dist2 gamma over the weight chain's range: the median distance among finite rows gets ``u``"""
    from scann import _hip

    ok = np.nonzero(np.isfinite(rows).all(1) & (np.abs(rows) < 1e10).all(1))[0][:96]
    d2 = _hip.knn_dist2_matrix(rows[ok], rows[ok]) if len(ok) else np.zeros((0, 0), np.float32)
    med = float(np.median(d2[d2 > 0])) if (d2 > 0).any() else 1.0
    return float(np.float32(u / med))


def same_peaks(got, want, label):
    assert np.array_equal(got["sum"], want["sum"]), label + ": sums"
    assert np.array_equal(got["parent"], want["parent"]), label + ": parents"
    assert np.array_equal(_bits(got["delta2"]), _bits(want["delta2"])), label + ": delta2"


def queries_for(rows, nq, seed=0):
    """queries on and around rows of the pool, with the positions to leave out: a query's own row, another row, none"""
    rng = np.random.default_rng(seed + nq)
    pick = rng.integers(0, len(rows), nq)
    q = rows[pick].copy()
    q[1::2] += rng.standard_normal(q[1::2].shape).astype(np.float32) * np.float32(0.25)
    skip = np.where(np.arange(nq) % 3 == 0, pick, np.where(np.arange(nq) % 3 == 1, -1, (pick + 1) % len(rows))).astype(np.int32)
    return q, skip


def check_pool(eng, rows, gamma, label, nq=150):
    """both device calls on an index of ``rows`` against the twins; returns the device's peaks"""
    from scann import _hip

    ix = make_index(eng, rows)
    try:
        got = eng.index_peaks(ix, gamma)
        want = _hip.peaks_host(rows, gamma)
        same_peaks(got, want, label)
        q, skip = queries_for(rows, nq)
        for s in (None, skip):
            assert np.array_equal(eng.index_density(ix, q, gamma, s), _hip.density_host(rows, q, gamma, s)), label + ": density"
        assert np.array_equal(eng.index_density(ix, rows, gamma, np.arange(len(rows))), got["sum"]), label + ": the self-join as queries"
    finally:
        ix.free()
    el = got["sum"] >= 0
    print("%s: gamma %.3g, sums in [%d, %d], %d distinct, %d roots, %d ineligible" % (
        label, gamma, got["sum"][el].min() if el.any() else -1, got["sum"].max(), len(np.unique(got["sum"])), int(((got["parent"] < 0) & el).sum()),
        int((~el).sum())))
    assert int(((got["parent"] < 0) & el).sum()) == (1 if el.any() else 0)
    return got


# ---- 1. the kernels against the twins ----

@pytest.mark.parametrize("dim", [1, 3, 128, 130, 1024])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 127, 128, 129, 1000, 5000])
def test_kernels_equal_the_host_twins(engine, N, dim):
    rows = random_rows(N, dim)
    got = check_pool(engine, rows, gamma_for(rows), "N %d dim %d" % (N, dim))
    if N >= 100 and dim > 1:
        assert len(np.unique(got["sum"])) > N // 2  # the sums tell the rows apart: the parents were not decided by position alone
        assert (got["delta2"][N // 2 + 1:N // 2 + 4] == 0).all()  # random_rows' duplicates follow their earlier copy


def test_planted_ties_and_non_finite_rows(engine):
    rows = random_rows(700, 130, seed=12)
    gamma = gamma_for(rows)
    rows[100:140] = rows[7]           # 41 coincident rows: equal sums, ties by position
    rows[300:364] = rows[299]         # a whole tile of them
    rows[13, 129] = np.nan
    rows[400, 128] = np.inf
    rows[401, 0] = -np.inf
    rows[401, 5] = np.nan
    rows[500] = np.float32(3e19)      # finite: every distance overflows to +inf, every term is 0
    rows[501] = np.float32(-3e19)
    rows[502, 64] = np.float32(1e6)   # far, not overflowing
    got = check_pool(engine, rows, gamma, "planted")
    for i in (13, 400, 401):
        assert got["sum"][i] == -1 and got["parent"][i] == -1 and got["delta2"][i] == np.inf
    assert got["sum"][500] == 0 and got["sum"][501] == 0 and got["delta2"][500] == np.inf and got["parent"][500] >= 0  # a parent at +inf
    assert (got["sum"][100:140] == got["sum"][7]).all() and (got["parent"][100:140] == 7).all()
    assert (got["parent"][300:364] == 299).all() and (got["delta2"][300:364] == 0).all()
    # small integers, where plain NumPy gives the chain's bits: the restated definition and its certificate
    import kcenter_ref
    from scann import _hip

    ints = peaks_ref.small_integer_rows(200, 9, seed=2)
    ints[50:60] = ints[3]
    ints[77, 2] = np.nan
    g = check_pool(engine, ints, 0.02, "small integers")
    sums, parent, delta2, _ = peaks_ref.peaks(ints, kcenter_ref.exact_dist2, _hip.rbf_weight, 0.02)
    assert [int(s) for s in g["sum"]] == sums and np.array_equal(g["parent"], parent) and np.array_equal(_bits(g["delta2"]), _bits(delta2))
    peaks_ref.certificate(ints, g["sum"], g["parent"], g["delta2"], kcenter_ref.exact_dist2)
    same = np.tile(ints[:1], (130, 1))
    g = check_pool(engine, same, 0.5, "all coincident")
    assert (g["sum"] == 129 * 2 ** 30).all() and g["parent"][0] == -1 and (g["parent"][1:] == 0).all()
    far = check_pool(engine, ints, 200.0, "vanishing weights")
    assert set(np.unique(far["sum"]).tolist()) <= {-1, 0, 2 ** 30, 10 * 2 ** 30} and (far["sum"] == 0).sum() > 150  # ints[3] has ten copies


def test_an_empty_pool(engine):
    ix = engine.index_create(8)
    try:
        r = engine.index_peaks(ix, 0.5)
        assert r["sum"].shape == (0,) and r["parent"].shape == (0,)
        q = np.ones((3, 8), np.float32)
        q[1, 2] = np.nan
        assert list(engine.index_density(ix, q, 0.5)) == [0, -1, 0]
        assert engine.index_density(ix, np.zeros((0, 8), np.float32), 0.5).shape == (0,)
    finally:
        ix.free()


# ---- 2. two storage chunks ----

@pytest.fixture(scope="module")
def two_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns"""
    rows = random_rows(17000, 1024)
    ix = make_index(engine, rows)
    yield rows, ix
    ix.free()


def test_density_over_two_chunks(engine, two_chunks):
    from scann import _hip

    rows, ix = two_chunks
    gamma = gamma_for(rows, u=3.0)
    q, skip = queries_for(rows, 300)
    q[0], q[1], q[2] = rows[16383], rows[16384], rows[16999]  # queries on either side of the chunk boundary and on the last row
    skip[:3] = [16383, -1, 16999]
    got = engine.index_density(ix, q, gamma, skip)
    assert np.array_equal(got, _hip.density_host(rows, q, gamma, skip))
    assert np.array_equal(engine.index_density(ix, q, gamma), _hip.density_host(rows, q, gamma))
    assert (got > 0).all()


def test_peaks_over_two_chunks(engine, two_chunks):
    """the self-join of all 17,000 rows: query tiles and row ranges both cross the chunk boundary"""
    from scann import _hip

    rows, ix = two_chunks
    gamma = gamma_for(rows, u=3.0)
    got = engine.index_peaks(ix, gamma)
    same_peaks(got, _hip.peaks_host(rows, gamma), "17,000 x 1,024")
    assert len(np.unique(got["sum"])) > 16000 and int((got["parent"] < 0).sum()) == 1
    assert (got["parent"][16384:] < 16384).any() and (got["parent"][:16384] >= 16384).any()  # parents on the other side of the boundary


# ---- 3. invariance ----

def test_results_do_not_depend_on_how_the_pool_was_built(engine):
    dim, N = 130, 3000
    rows = random_rows(N, dim, seed=9)
    gamma = gamma_for(rows)
    q, skip = queries_for(rows, 200)
    one = make_index(engine, rows)
    first = engine.index_peaks(one, gamma), engine.index_density(one, q, gamma, skip)
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
        same_peaks(engine.index_peaks(many, gamma), first[0], "many adds")
        assert np.array_equal(engine.index_density(many, q, gamma, skip), first[1])
        same_peaks(engine.index_peaks(one, gamma), first[0], "repeat")
    finally:
        junk[1].free()
        one.free()
        many.free()


# ---- 4. end to end ----

def level_rows_of(eng, rb):
    """(y, ga, {"structure": bf_property rows, "atom": after_Lc rows}) of a plain forward of the resident batch"""
    from scann import _hip

    eng.set_outputs(after_lc=True, bf_property=True)
    try:
        eng.forward_resident(rb)
        y, ga = eng.download(rb)
        return y, ga, {"structure": eng.read_output(rb, _hip.OUT_BF_PROPERTY), "atom": eng.read_output(rb, _hip.OUT_AFTER_LC)}
    finally:
        eng.set_outputs()


def check_density_batch(model, data, label, pools=None):
    """density_batch == read_output -> density_host against the pool's rows; y and ga those of a plain forward"""
    from scann import _hip

    eng = model.engine
    rb = eng.upload(_hip.pack_inputs(data))
    y, ga, level_rows = level_rows_of(eng, rb)
    for level in ("structure", "atom"):
        lvl, rows = _hip.KNN_LEVELS[level], level_rows[level]
        pool_rows = np.concatenate([rows[::2], rows[:5] + np.float32(0.125), random_rows(300, rows.shape[1], seed=5) * np.float32(0.01) + rows[0]])
        gamma = gamma_for(pool_rows, u=2.0)
        ix = make_index(eng, pool_rows)
        try:
            got = eng.density_batch(ix, rb, lvl, gamma)
        finally:
            ix.free()
        want = _hip.density_host(pool_rows, rows, gamma)
        assert np.array_equal(got["sum"], want), "%s %s" % (label, level)
        assert np.array_equal(_bits(got["y"]), _bits(y)) and np.array_equal(_bits(got["ga"]), _bits(ga)), "%s %s: y, ga" % (label, level)
        assert (got["sum"][::2] >= 2 ** 30).all()  # every second query lies on a pool row
        print("%s %s: %d queries of %d columns against %d rows, sums in [%d, %d]" % (
            label, level, len(rows), rows.shape[1], len(pool_rows), got["sum"].min(), got["sum"].max()))
    rb.free()


E2E = {"qm9": 40, "mp2018": 24}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_density_peaks_of_a_model_is_the_twin_on_its_rows(hip_lib, kind, level, tmp_path):
    from scann import _hip
    from scann.models import LatentPeaks
    from scann.models import latent_index as li

    n = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n, seed=0)
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    rows, ids, atoms = index.rows()
    res, pk = model.density_peaks(index, k=3)
    want, pk_w = li.density_peaks_rows_host(rows, k=3, ids=ids, atoms=atoms, level=level)
    print("%s %s: %d rows, bandwidth %.4g, sizes %s, decision %s" % (kind, level, len(rows), res["bandwidth"], res["size"], res["decision"][:5]))
    assert res["bandwidth"] == want["bandwidth"] and res["gamma"] == want["gamma"]
    for key in ("label", "parent", "sum", "centre_position", "centre_id", "centre_atom", "size"):
        assert np.array_equal(res[key], want[key]), key
    for key in ("density", "delta", "decision"):
        assert np.array_equal(res[key].view(np.uint64), want[key].view(np.uint64)), key
    r = model.engine.index_peaks(index._ix, res["gamma"])
    same_peaks(r, _hip.peaks_host(rows, res["gamma"]), "the twin")
    assert np.array_equal(r["sum"], res["sum"]) and np.array_equal(r["parent"], res["parent"])
    assert np.array_equal(np.sqrt(r["delta2"].astype(np.float64)), res["delta"])
    peaks_ref.certificate(rows, r["sum"], r["parent"], r["delta2"], _hip.knn_dist2_matrix)
    assert np.array_equal(pk.label, pk_w.label) and np.array_equal(pk.ids, ids) and np.array_equal(pk.atoms, atoms) and pk.level == level
    assert res["label"].min() == 0 and res["size"].sum() == len(rows) and res["label"][res["centre_position"][0]] == 0
    # the host route, thresholds, data instead of an index, save and load
    host, _ = index.density_peaks(k=3, route="host")
    assert np.array_equal(host["label"], res["label"]) and np.array_equal(host["sum"], res["sum"])
    thr, _ = index.density_peaks(bandwidth=res["bandwidth"], min_density=0.0, min_delta=float(np.sort(res["delta"][np.isfinite(res["delta"])])[-2]))
    assert len(thr["size"]) >= 3 and thr["centre_position"][0] == res["centre_position"][0]  # the root and the two rows farthest from anything denser
    direct, _ = model.density_peaks(data, level=level, k=3, batch_size=16, ids=np.arange(n) * 2 + 1)
    assert np.array_equal(direct["label"], res["label"]) and np.array_equal(direct["centre_id"], res["centre_id"])
    pk.save(str(tmp_path / "pk.npz"))
    back = LatentPeaks.load(model, str(tmp_path / "pk.npz"))
    pos = model.engine.index_query(index._ix, rows, 1)["position"][:, 0]
    assert np.array_equal(back.label_of(pos), res["label"][pos])
    # the density of the model's own inputs under its own index: every query lies on a row
    d = model.density(data, index, res["bandwidth"], batch_size=16)
    pkd = model.density(_hip.pack_inputs(data), index, res["bandwidth"], batch_size=16)
    y, ga = model.predict(data)
    assert np.array_equal(_bits(d["predict_property"][:, 0]), _bits(y[:, 0])) and np.array_equal(_bits(pkd["predict_property"]), _bits(d["predict_property"]))
    assert np.array_equal(pkd["sum"], _hip.density_host(rows, rows, res["gamma"])) and np.array_equal(pkd["sum"], res["sum"] + 2 ** 30)
    assert np.array_equal(pkd["density"], np.ldexp(pkd["sum"].astype(np.float64), -30) / len(rows))
    if level == "atom":
        amask = np.asarray(data["atom_mask"]).reshape(d["sum"].shape) != 0
        assert np.array_equal(d["sum"], _hip.repad_atoms(pkd["sum"], data["atom_mask"], -1)) and d["density"].dtype == np.float64
        assert np.array_equal(d["density"][amask].view(np.uint64), li.density_of_sums(d["sum"][amask], len(index)).view(np.uint64))
        assert np.array_equal(d["density"][amask].view(np.uint64), pkd["density"].view(np.uint64)) and not d["density"][~amask].any()
    else:
        assert np.array_equal(d["sum"], pkd["sum"]) and d["density"].dtype == np.float64
        assert np.array_equal(d["density"].view(np.uint64), li.density_of_sums(d["sum"], len(index)).view(np.uint64))
    index.free()


@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_density_batch_is_a_forward_and_the_twin(hip_lib, kind):
    cfg, w, data, model = setup(kind=kind, n=E2E[kind], seed=0)
    check_density_batch(model, data, kind)


def test_density_batch_on_a_generic_width_handle(hip_lib):
    """rows of 30 and 96 columns, the first no multiple of 4"""
    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    check_density_batch(model, data, "generic")
    index = model.build_index(data, level="structure")
    res, _ = model.density_peaks(index, k=2, bandwidth=1.0)
    from scann import _hip

    r = model.engine.index_peaks(index._ix, res["gamma"])
    same_peaks(r, _hip.peaks_host(index.rows()[0], res["gamma"]), "generic width")
    assert np.array_equal(r["sum"], res["sum"]) and np.array_equal(r["parent"], res["parent"]) and len(res["size"]) == 2
    index.free()


# ---- 5. state ----

def test_nothing_else_changes(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool, rb, rows = u.eng, u.pool, u.rb, u.rows[0]
        gamma = gamma_for(rows)
        first = eng.index_peaks(pool, gamma)
        d_first = eng.index_density(pool, rows[:50], gamma)
        spool = make_index(eng, np.random.default_rng(0).standard_normal((70, 128)).astype(np.float32))

        def same(r):
            same_peaks(r[0], first, "repeat")
            assert np.array_equal(r[1], d_first)

        u.repeat(lambda: (eng.index_peaks(pool, gamma), eng.index_density(pool, rows[:50], gamma)), same, 5, 16 << 20)
        u.check()
        # density_batch: y is the plain forward's; the selection is put back
        r = eng.density_batch(spool, rb, _hip.OUT_BF_PROPERTY, 0.01)
        assert np.array_equal(_bits(r["y"]), _bits(u.y_first)) and (r["sum"] > 0).all()
        u.reforward()
        spool.free()


def test_training_handle(hip_lib):
    """after two training steps the calls on the training handle equal the host twins' and an inference handle's, and weights, gradients
    and the following (deterministic) step -- the Adam state entered it -- are those of a twin that never made the calls"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows = random_rows(900, 128, seed=8)
    gamma = gamma_for(rows)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, rows)
        same_peaks(eng.index_peaks(ix, gamma), _hip.peaks_host(rows, gamma), "training handle")
        inf_model, rb2 = inference()
        inf = inf_model.engine
        ix2 = make_index(inf, rows)
        for level in (_hip.OUT_BF_PROPERTY, _hip.OUT_AFTER_LC):
            db = [e.density_batch(x, b, level, gamma) for e, x, b in ((eng, ix, rb), (inf, ix2, rb2))]
            same_arrays(db[0], db[1], "training against inference handle")
        ix.free()
        ix2.free()

    training_twin(cfg, w, pk, calls)


# ---- 6. errors, the CLI ----

def test_errors_name_what_is_wrong(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows = random_rows(5, 4, seed=0)
    pool, foreign, narrow = make_index(eng, rows), make_index(other.engine, rows), make_index(eng, rows)
    P = _hip._ptr
    sums, parent, delta2 = np.full(5, 7, np.int64), np.full(5, 7, np.int32), np.full(5, 7, np.float32)

    def message():
        return (eng.lib.scann_last_error(eng._h) or b"").decode()

    def dens(p=pool, q=rows, nq=5, gamma=0.5, s=sums):
        return eng.lib.scann_index_density(eng._h, None if p is None else p._h, P(q), nq, None, gamma, P(s))

    def peaks(p=pool, gamma=0.5, s=sums, par=parent, d=delta2):
        return eng.lib.scann_index_peaks(eng._h, None if p is None else p._h, gamma, P(s), P(par), P(d))

    rb = eng.upload(_hip.pack_inputs(data))
    spool = make_index(eng, np.zeros((3, 128), np.float32))
    free0, _ = eng.device_memory()  # (the batch and every index are there already: what follows must take nothing)
    assert dens(p=None) == -1 and "scann_index_density: null handle or pool" in message()
    assert dens(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert dens(q=None) == -1 and "q is null" in message()
    assert dens(s=None) == -1 and "sums is null" in message()
    assert dens(nq=-1) == -1 and "nq -1 outside" in message()
    assert peaks(p=None) == -1 and "scann_index_peaks: null handle or pool" in message()
    assert peaks(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert peaks(s=None) == -1 and "sums is null" in message()
    assert peaks(par=None) == -1 and "parent is null" in message()
    assert peaks(d=None) == -1 and "delta2 is null" in message()
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert dens(gamma=g) == -1 and "gamma must be finite and > 0" in message(), g
        assert peaks(gamma=g) == -1 and "gamma must be finite and > 0" in message(), g

    def batch(ix=spool, b=rb, level=_hip.OUT_BF_PROPERTY, gamma=0.5, s=sums):
        return eng.lib.scann_index_density_batch(eng._h, None if ix is None else ix._h, None if b is None else b._h, level, gamma, None, None, P(s))

    assert batch(ix=None) == -1 and "scann_index_density_batch: null argument" in message()
    assert batch(b=None) == -1 and "null argument" in message()
    assert batch(ix=foreign) == -1 and "index belongs to another handle" in message()
    assert batch(level=9) == -1 and "level must be" in message() and "got 9" in message()
    assert batch(ix=narrow) == -1 and "the index holds rows of 4 columns, the model's dense_out is 128" in message()
    assert batch(gamma=0.0) == -1 and "gamma must be finite and > 0" in message()
    assert batch(s=None) == -1 and "sums is null" in message()
    # nothing was written, nothing stays allocated
    assert (sums == 7).all() and (parent == 7).all() and (delta2 == 7).all() and free0 - eng.device_memory()[0] <= 8 << 20
    assert dens() == 0 and peaks() == 0 and batch() == 0
    rb.free()
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError, match="gamma"):
        eng.index_peaks(pool, 0.0)
    with pytest.raises(ValueError, match="q must"):
        eng.index_density(pool, np.zeros((2, 5), np.float32), 0.5)
    with pytest.raises(ValueError, match="skip_pos"):
        eng.index_density(pool, rows, 0.5, np.zeros(4, np.int32))
    lat = model.build_index(data)
    for kw, word in ((dict(), "exactly one"), (dict(k=2, min_density=0.0, min_delta=0.0), "exactly one"), (dict(k=0), "k must"),
                     (dict(k=5), "k = 5"), (dict(k=2, bandwidth=0.0), "bandwidth"), (dict(k=2, neighbours=40), "neighbours"),
                     (dict(k=2, route="gpu"), "route")):
        with pytest.raises(ValueError, match=word):
            lat.density_peaks(**kw)
    with pytest.raises(ValueError):
        other.density_peaks(lat, k=2)  # another model's index
    with pytest.raises(ValueError, match="LatentIndex"):
        model.density(data, "an index", 1.0)
    with pytest.raises(ValueError, match="bandwidth"):
        model.density(data, lat, 0.0)
    with pytest.raises(ValueError, match="level"):
        model.density_peaks(data, level="bond", k=2)
    for ix in (pool, foreign, narrow, spool, lat):
        ix.free()


def test_cli_writes_and_loads_peaks(hip_lib, tmp_path):
    """predict_model.py --peaks writes peaks_<target>.pickle and, with --peaks-out, peaks.npz, which loads back; --density pickles the
    density under a saved index; the other files' bytes are those of a run without the flags"""
    import yaml

    from scann.models import SCANN, LatentPeaks
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
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    pool.save(str(tmp_path / "index.npz"))
    want, pk = scann.density_peaks(pool, k=3)
    r = subprocess.run(cli + ["--peaks", "3", "--peaks-out", str(tmp_path / "peaks.npz"), "--density", str(tmp_path / "index.npz"),
                              "--density-bandwidth", repr(want["bandwidth"])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"peaks_homo.pickle", "density_homo.pickle"}
    got = pickle.load(open(out / "peaks_homo.pickle", "rb"))
    assert sorted(got) == sorted(list(want) + ["id", "atom"])
    for key in ("label", "parent", "sum", "centre_position", "centre_id", "size", "decision"):
        assert np.array_equal(got[key], want[key]), key
    assert got["bandwidth"] == want["bandwidth"] and "bandwidth" in r.stdout and "cluster    0" in r.stdout
    saved = LatentPeaks.load(scann.model, str(tmp_path / "peaks.npz"))
    assert np.array_equal(saved.label, pk.label) and np.array_equal(saved.ids, pk.ids) and saved.bandwidth == pk.bandwidth and saved.k == 3
    per = pickle.load(open(out / "density_homo.pickle", "rb"))
    inputs, _ = data[0]
    first = scann.density(inputs, pool, want["bandwidth"])
    amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
    assert len(per) == n and sorted(per[0]) == ["density", "predict_property", "sum"]
    assert np.array_equal(per[0]["sum"], first["sum"][0][amask[0]]) and (per[0]["sum"] >= 2 ** 30).all()
    pool.free()

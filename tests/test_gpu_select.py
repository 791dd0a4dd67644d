"""GPU tests of the greedy k-center selection (scann_index_select through Engine.index_select, LatentIndex.select,
HipModel.select_diverse).  Every comparison is exact: positions equal, radius2 bit for bit.

1. Kernel against the host twin (scann_kcenter_host) on random pools: N below one tile of 256 rows, not a multiple of it, more than one
   storage chunk; dim in {1, 3, 128, 130, 1024}; with and without a reference; m from 1 to beyond N.
2. The planted cases of tests/test_select_host.py on the device.
3. Invariance: one add or many, and after unrelated indices were created and freed.
4. End to end on the qm9 and mp2018 fixtures at both levels: select_diverse == kcenter_host on the rows the indices hold, and the
   independent certificate of tests/kcenter_ref.py from the full distance matrices.
5. Non-interference: pool, reference, weights, selected outputs, the batch's last y, a training handle's state; device memory.
6. Errors name what is wrong.  7. The CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import kcenter_ref
import scann_oracle as so
from analysis_checks import _bits, make_index, padded, scan_edge_rows, setup, training_twin, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def check_exact(eng, rows, ref, m, stop=0.0, ids=None, atoms=None, label=""):
    """the device's selection against the host twin's: count, positions, radius2 bits, ids, atoms and the tails"""
    from scann import _hip

    pool = make_index(eng, rows, ids, atoms)
    rix = None if ref is None else make_index(eng, ref)
    try:
        got = eng.index_select(pool, rix, m, stop)
    finally:
        pool.free()
        if rix is not None:
            rix.free()
    want = _hip.kcenter_host(rows, ref, m, stop)
    cnt = want["count"]
    n_bad = int((got["position"] != want["position"]).sum())
    print("%s: N %d, dim %d, reference %s, m %d, stop %g: %d picks (host %d), %d of %d positions differ" % (
        label, len(rows), rows.shape[1], "none" if ref is None else len(ref), m, stop, got["count"], cnt, n_bad, m))
    assert got["count"] == cnt, label
    assert np.array_equal(got["position"], want["position"]), label
    assert np.array_equal(_bits(got["radius2"]), _bits(want["radius2"])), label
    ids = np.arange(len(rows), dtype=np.int64) if ids is None else ids
    atoms = np.full(len(rows), -1, np.int32) if atoms is None else atoms
    p = got["position"][:cnt]
    assert np.array_equal(got["id"][:cnt], ids[p]) and np.array_equal(got["atom"][:cnt], atoms[p]), label
    assert np.all(got["position"][cnt:] == -1) and np.all(got["id"][cnt:] == -1) and np.all(got["atom"][cnt:] == -1), label
    assert np.all(np.isposinf(got["radius2"][cnt:])), label
    r = got["radius2"][:cnt]
    assert np.all(r[1:] <= r[:-1]), label
    return got


# (N, dim, reference rows or 0, the m's).  A tile is 256 rows; a storage chunk holds 64 MiB of rows, i.e. 16,384 rows of 1,024 columns:
# 17,000 x 1,024 spans two chunks.  m runs from 1 to beyond N where N is small
RANDOM_CASES = [(1, 128, 0, (1, 3)), (1, 3, 5, (2,)), (100, 128, 0, (1, 7, 103)), (100, 130, 30, (1, 100)), (255, 1, 0, (300,)), (256, 3, 40, (9, 256)),
                (257, 130, 0, (5, 260)), (1000, 128, 200, (1, 64)), (1000, 3, 0, (1003,)), (1000, 1, 64, (50,)), (5000, 130, 300, (33,)),
                (20000, 128, 0, (40,)), (20000, 3, 1000, (25,)), (600, 1024, 70, (12, 601)), (17000, 1024, 0, (20,)), (17000, 1024, 50, (20,))]


@pytest.mark.parametrize("N,dim,nr,ms", RANDOM_CASES, ids=["N%d_d%d_R%d" % c[:3] for c in RANDOM_CASES])
def test_kernel_exact_on_random_pools(engine, N, dim, nr, ms):
    rng = np.random.default_rng(N * 5 + dim * 3 + nr)
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    if N >= 100:
        rows[N // 2:N // 2 + 4] = rows[3]  # ties
    ref = rng.standard_normal((nr, dim)).astype(np.float32) if nr else None
    ids = rng.integers(0, 1 << 40, N).astype(np.int64)
    atoms = rng.integers(-1, 30, N).astype(np.int32)
    for m in ms:
        got = check_exact(engine, rows, ref, m, ids=ids, atoms=atoms, label="random")
        assert got["count"] == min(m, N)
    if ref is None:
        assert got["position"][0] == 0 and np.isposinf(got["radius2"][0])


def test_kernel_exact_on_small_integers(engine):
    """many exact ties: the order by position decides, on the device as in NumPy"""
    rng = np.random.default_rng(4)
    rows = rng.integers(-4, 5, (3000, 3)).astype(np.float32)
    ref = rng.integers(-4, 5, (20, 3)).astype(np.float32)
    for r in (None, ref):
        got = check_exact(engine, rows, r, 400, label="integers")
        pos, rad, cnt = kcenter_ref.select(rows, r, 400, 0.0, kcenter_ref.exact_dist2)
        assert got["count"] == cnt and np.array_equal(got["position"], pos) and np.array_equal(_bits(got["radius2"]), _bits(rad))


def test_edges_of_the_eligibility_scan(engine):
    """with m beyond N every eligible row is picked, and no other"""
    for label, rows in scan_edge_rows():
        ok = np.isfinite(rows).all(axis=1)
        got = check_exact(engine, rows, None, len(rows) + 2, label=label)
        assert sorted(got["position"][:got["count"]].tolist()) == np.flatnonzero(ok).tolist(), label


def test_planted_cases_on_the_device(engine):
    from test_select_host import planted

    rng = np.random.default_rng(11)
    rows, bad, dup = planted(rng)
    n = len(rows)
    got = check_exact(engine, rows, None, n + 10, label="planted")
    cnt = got["count"]
    assert cnt == n - len(bad)
    pos, r2 = got["position"][:cnt], got["radius2"][:cnt]
    assert not set(bad) & set(pos.tolist()) and len(set(pos.tolist())) == cnt
    group = [5] + dup
    assert [p for p in pos if p in group][0] == 5 and pos[-3:].tolist() == sorted(dup) and not r2[-3:].any() and np.all(r2[:-3] > 0)
    got = check_exact(engine, rows, rows[5:6] + 0, n, label="planted, reference")
    assert got["position"][got["count"] - 4:got["count"]].tolist() == sorted(group) and not got["radius2"][got["count"] - 4:got["count"]].any()
    # a wide pool with non-finite values in a late column and in the padding's neighbour (dim 130: stride 132)
    wide = (rng.standard_normal((700, 130)) * 2).astype(np.float32)
    wide[13, 129] = np.nan
    wide[300, 128] = np.inf
    wide[699, 0] = -np.inf
    got = check_exact(engine, wide, wide[40:45] + np.float32(0.5), 700, label="planted, wide")
    assert got["count"] == 697 and not {13, 300, 699} & set(got["position"].tolist())
    # all rows equal
    same = np.tile(np.float32([1.5, -2.0, 0.25]), (300, 1))
    got = check_exact(engine, same, None, 310, label="all equal")
    assert got["count"] == 300 and got["position"][:300].tolist() == list(range(300)) and np.isposinf(got["radius2"][0]) and not got["radius2"][1:300].any()
    assert check_exact(engine, same, None, 310, stop=1e-6, label="all equal, stop")["count"] == 1
    # only non-finite rows: nothing to pick; an empty pool returns 0
    assert check_exact(engine, np.full((5, 4), np.nan, np.float32), None, 3, label="no eligible row")["count"] == 0
    assert check_exact(engine, np.zeros((0, 4), np.float32), None, 3, label="empty pool")["count"] == 0
    # an empty reference index is no reference; a reference row with a NaN is ignored; a reference of such rows only likewise
    rows = rng.standard_normal((500, 20)).astype(np.float32)
    ref = rng.standard_normal((25, 20)).astype(np.float32)
    got = check_exact(engine, rows, np.zeros((0, 20), np.float32), 6, label="empty reference")
    assert got["position"][0] == 0 and np.isposinf(got["radius2"][0])
    base = check_exact(engine, rows, ref, 30, label="reference")
    dirty = np.concatenate([ref[:10], np.full((1, 20), 1.0, np.float32), ref[10:]])
    dirty[10, 4] = np.nan
    got = check_exact(engine, rows, dirty, 30, label="reference with a NaN row")
    assert np.array_equal(got["position"], base["position"]) and np.array_equal(_bits(got["radius2"]), _bits(base["radius2"]))
    got = check_exact(engine, rows, np.full((2, 20), np.nan, np.float32), 5, label="NaN reference")
    assert got["position"][0] == 0 and np.isposinf(got["radius2"][0])
    perm = check_exact(engine, rows, ref[rng.permutation(25)], 30, label="reference permuted")
    assert np.array_equal(perm["position"], base["position"]) and np.array_equal(_bits(perm["radius2"]), _bits(base["radius2"]))


def test_stop_rule_on_the_device(engine):
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((700, 12)).astype(np.float32)
    ref = rng.standard_normal((10, 12)).astype(np.float32)
    full = check_exact(engine, rows, ref, 700, label="no stop")
    r2 = full["radius2"]
    for cut in (1, 2, 50, 699):
        assert r2[cut] < r2[cut - 1]
        for stop in (np.float32(0.5) * (r2[cut - 1] + r2[cut]), r2[cut - 1]):
            got = check_exact(engine, rows, ref, 700, stop=float(stop), label="stop")
            assert got["count"] == cut and np.array_equal(got["position"][:cut], full["position"][:cut])
    assert check_exact(engine, rows, ref, 700, stop=float(np.nextafter(r2[0], np.float32(np.inf))), label="stop above all")["count"] == 0
    assert check_exact(engine, rows, ref, 700, stop=-3.0, label="stop <= 0")["count"] == 700
    assert check_exact(engine, rows, None, 700, stop=1e30, label="stop, no reference")["count"] == 1


def test_invariance_of_how_the_indices_were_built(engine):
    rng = np.random.default_rng(9)
    dim, N = 130, 3000
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    rows[1500:1510] = rows[3]
    ref = rng.standard_normal((500, dim)).astype(np.float32)
    one, many, r_one, r_many = (engine.index_create(dim) for _ in range(4))
    try:
        engine.index_add(one, rows)
        engine.index_add(r_one, ref)
        at = 0
        for step in [1, 63, 64, 65, 7, 1000, 3, 500, 255, 257]:
            engine.index_add(many, rows[at:at + step])
            at += step
        while at < N:
            engine.index_add(many, rows[at:at + 311])
            at += 311
        for at in range(0, 500, 77):
            engine.index_add(r_many, ref[at:at + 77])
        assert len(one) == len(many) == N and len(r_one) == len(r_many) == 500
        a = engine.index_select(one, r_one, 200)
        # unrelated indices come and go in between (the workspace and the chunks come from the same block cache)
        for d in (64, 130, 7):
            tmp = make_index(engine, rng.standard_normal((900, d)).astype(np.float32))
            engine.index_select(tmp, None, 5)
            tmp.free()
        for p, r in ((many, r_many), (one, r_many), (many, r_one), (one, r_one)):
            b = engine.index_select(p, r, 200)
            assert b["count"] == a["count"] == 200
            for key in ("position", "id", "atom"):
                assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(_bits(a["radius2"]), _bits(b["radius2"]))
        # a shorter run is a prefix of a longer one
        c = engine.index_select(one, r_one, 37)
        assert np.array_equal(c["position"], a["position"][:37]) and np.array_equal(_bits(c["radius2"]), _bits(a["radius2"][:37]))
    finally:
        for ix in (one, many, r_one, r_many):
            ix.free()


# ---- end to end ----

E2E = {"qm9": (64, 24), "mp2018": (24, 8)}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_select_diverse_is_the_host_selection_on_the_models_rows(hip_lib, kind, level):
    from scann import _hip

    n_p, n_r = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n_p, seed=0)
    labelled = padded(kind, n_r, 1, cfg)
    pool = model.build_index(data, level=level, batch_size=16, ids=np.arange(n_p) * 2 + 1)
    ref = model.build_index(labelled, level=level)
    rows, ids, atoms = pool.rows()
    rrows = ref.rows()[0]
    m = min(40, len(rows) + 3)
    for reference, rr in ((ref, rrows), (None, None)):
        got = model.select_diverse(pool, m, reference=reference)
        want = _hip.kcenter_host(rows, rr, m)
        cnt = want["count"]
        assert got["count"] == cnt == min(m, len(rows))
        assert np.array_equal(got["position"], want["position"][:cnt])
        assert np.array_equal(_bits(got["radius"]), _bits(np.sqrt(want["radius2"][:cnt])))
        assert np.array_equal(got["neighbor_id"], ids[got["position"]]) and np.array_equal(got["atom"], atoms[got["position"]])
        if level == "structure":
            assert np.all(got["atom"] == -1)
        # the certificate, from the full distance matrices
        raw = model.engine.index_select(pool._ix, None if reference is None else reference._ix, m)
        kcenter_ref.certificate(rows, rr, raw["position"], raw["radius2"], raw["count"], _hip.knn_dist2_matrix, m=m)
        assert np.array_equal(raw["position"][:cnt], got["position"])
    # data instead of indices: indexed for the call and freed; the same picks (ids 0 .. n-1 in input order there)
    direct = model.select_diverse(data, m, reference=labelled, level=level, batch_size=16)
    again = model.select_diverse(pool, m, reference=ref)
    assert np.array_equal(direct["position"], again["position"]) and np.array_equal(_bits(direct["radius"]), _bits(again["radius"]))
    assert np.array_equal(direct["neighbor_id"] * 2 + 1, again["neighbor_id"]) and np.array_equal(direct["atom"], again["atom"])
    # a threshold: the run is the prefix whose radii are not below it
    stop = float(again["radius"][len(again["radius"]) // 2])
    cut = model.select_diverse(pool, m, reference=ref, stop_distance=stop)
    raw = model.engine.index_select(pool._ix, ref._ix, m)
    keep = int((raw["radius2"][:raw["count"]] >= np.float32(stop) * np.float32(stop)).sum())  # (the threshold is squared in fp32 for the call)
    assert 1 <= keep <= again["count"]
    assert cut["count"] == keep and np.array_equal(cut["position"], again["position"][:keep])
    pool.free()
    ref.free()


# ---- state, errors ----

def test_nothing_else_changes(hip_lib):
    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool = u.eng, u.pool
        ref = make_index(eng, u.rows[0][:50] + np.float32(0.125))
        r0 = eng.index_read(ref)
        first = eng.index_select(pool, ref, 64)

        def call():
            r = eng.index_select(pool, ref, 64)
            eng.index_select(pool, None, 3, 0.5)
            return r

        def same(r):
            assert np.array_equal(r["position"], first["position"]) and np.array_equal(_bits(r["radius2"]), _bits(first["radius2"]))

        u.repeat(call, same, 20, 16 << 20)
        for a, b in zip(r0, eng.index_read(ref)):  # the reference index as well
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert len(ref) == 50
        ref.free()


def test_training_handle(hip_lib):
    """after two training steps a selection on the training handle equals the host twin's, and weights, gradients and the following
    (deterministic) step are those of a twin that never made the call"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rng = np.random.default_rng(2)
    rows = rng.standard_normal((900, 128)).astype(np.float32)
    ref = rng.standard_normal((60, 128)).astype(np.float32)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        check_exact(eng, rows, ref, 50, label="training handle")
        check_exact(eng, rows, None, 50, stop=100.0, label="training handle, stop")

    training_twin(cfg, w, pk, calls)


def test_generic_width_handle(hip_lib):
    """a handle of widths other than 128 / 8: rows of 32 and 96 columns"""
    from scann import _hip

    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=32)
    for level in ("structure", "atom"):
        ix = model.build_index(data, level=level, batch_size=4)
        rows = ix.rows()[0]
        got = ix.select(6)
        want = _hip.kcenter_host(rows, None, 6)
        assert got["count"] == want["count"] and np.array_equal(got["position"], want["position"][:got["count"]])
        assert np.array_equal(_bits(got["radius"]), _bits(np.sqrt(want["radius2"][:got["count"]])))
        ix.free()


def test_errors_name_what_is_wrong(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows = np.arange(12, dtype=np.float32).reshape(3, 4)
    pool, ref, narrow, foreign = make_index(eng, rows), make_index(eng, rows + 1), make_index(eng, rows[:, :3]), make_index(other.engine, rows)
    out = {"position": np.full(4, 7, np.int32), "radius2": np.full(4, 7, np.float32)}

    def call(p=pool, r=None, m=4, stop=0.0, pos=out["position"], handle=eng):
        return eng.lib.scann_index_select(handle._h, None if p is None else p._h, None if r is None else r._h, m, stop, _hip._ptr(pos), None, None,
                                          _hip._ptr(out["radius2"]))

    def message(e=eng):
        return (eng.lib.scann_last_error(e._h) or b"").decode()

    free0, _ = eng.device_memory()
    assert call(p=None) == -1 and "null" in message()
    assert call(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert call(r=foreign) == -1 and "reference belongs to another handle" in message()
    assert call(r=pool) == -1 and "the pool itself" in message()
    assert call(r=narrow) == -1 and "4 columns" in message() and "of 3" in message()
    assert call(m=0) == -1 and "m 0" in message()
    assert call(m=-5) == -1 and "m -5" in message()
    assert call(stop=float("nan")) == -1 and "NaN" in message()
    assert call(pos=None) == -1 and "pos is null" in message()
    assert call(handle=other.engine) == -1 and "another handle" in message(other.engine)
    # nothing was written, nothing was launched or allocated
    assert np.all(out["position"] == 7) and np.all(out["radius2"] == 7)
    assert free0 - eng.device_memory()[0] <= 1 << 20
    assert call(r=ref) == 3 and out["position"].tolist() == [0, 1, 2, -1]  # every row 4 away from the reference: by position
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError):
        eng.index_select(pool, pool, 2)
    with pytest.raises(ValueError):
        eng.index_select(pool, narrow, 2)
    for kw in (dict(m=0), dict(m=2, stop_dist2=float("nan"))):
        with pytest.raises(ValueError):
            eng.index_select(pool, None, **kw)
    lat = model.build_index(data)
    lat_atom = model.build_index(data, level="atom")
    for kw in (dict(m=0), dict(m=2, stop_distance=-1.0), dict(m=2, reference=lat), dict(m=2, reference=lat_atom)):
        with pytest.raises(ValueError):
            lat.select(**kw)
    with pytest.raises(ValueError):
        other.select_diverse(lat, 2)
    with pytest.raises(ValueError):
        model.select_diverse(data, 2, level="bond")
    for ix in (pool, ref, narrow, foreign, lat, lat_atom):
        ix.free()


def test_cli_writes_the_selection(hip_lib, tmp_path):
    """predict_model.py --select 6: selected_<target>.pickle, one dict in pick order; the other files' bytes are those of a run without
    the flag; --select-reference picks the dataset's structures farthest from a saved index"""
    import yaml

    from scann.models import SCANN, LatentIndex
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
    assert not os.path.exists(out / "selected_homo.pickle")
    listed = set(os.listdir(out))
    r = subprocess.run(cli + ["--select", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"selected_homo.pickle"}
    got = pickle.load(open(out / "selected_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, ids=data.indexes)
    want = scann.select_diverse(pool, 6)
    assert sorted(got) == ["atom", "count", "neighbor_id", "position", "radius"] and got["count"] == 6
    for k in ("position", "neighbor_id", "atom", "radius"):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    assert np.array_equal(got["neighbor_id"], np.asarray(data.indexes)[got["position"]]) and len(set(got["neighbor_id"].tolist())) == 6
    assert np.isposinf(got["radius"][0]) and np.all(np.diff(got["radius"]) <= 0)
    # a saved atom-level reference (the first 8 structures): the level is the reference's; the picks are the atoms farthest from it
    ref = scann.build_index(data[0][0], level="atom")
    ref.save(str(tmp_path / "labelled.npz"))
    r = subprocess.run(cli + ["--select", "5", "--select-reference", str(tmp_path / "labelled.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = pickle.load(open(out / "selected_homo.pickle", "rb"))
    atom_pool = scann.build_index(data, level="atom", ids=data.indexes)
    want = scann.select_diverse(atom_pool, 5, reference=LatentIndex.load(scann.model, str(tmp_path / "labelled.npz")))
    for k in ("position", "neighbor_id", "atom", "radius"):
        assert np.array_equal(got[k], want[k]), k
    assert got["count"] == 5 and np.all(got["atom"] >= 0) and np.all(np.isfinite(got["radius"]))
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f

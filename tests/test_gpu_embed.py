"""GPU tests of the neighbour embedding of a latent index (scann_embed_iterate, LatentIndex.embed / place, HipModel.fit_embedding /
place, predict_model.py --embed).  Every device comparison is an equality of bit patterns.
1. Engine.embed_iterate == the host twin (y, u, gain, the gradient and Z) either side of a block and of a span, three spans with a ragged
   last one, both phases' settings, a planted pair 1e10 apart (w * w subnormal), two coincident rows, a repeated call.
2. 6 iterations == 3 + 3; no iteration returns its inputs.
3. LatentIndex.embed by the device route == the host route == the all-host fit, on the planted blobs and on the qm9 fixture's after_Lc rows.
4. HipModel.fit_embedding on the qm9 and mp2018 fixtures at both levels and at a generic width; save, load, place; placed blob rows.
5. Nothing else changes, on an inference and a training handle; errors name the argument; the CLI."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import embed_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import _bits, setup, training_twin, untouched  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


def check_iterate(engine, st, n_iter, ex, mom, lr, label):
    from scann import _hip

    want = _hip.embed_iterate_host(*st, n_iter, ex, mom, lr, want_grad=True)
    got = engine.embed_iterate(*st, n_iter, ex, mom, lr, want_grad=True)
    print("%s: z %.17g, %d y values differ" % (label, got["z"], int((got["y"].view(np.uint32) != want["y"].view(np.uint32)).sum())))
    embed_ref.same_state(got, want, label)
    return got


# either side of a block (128) and of a span (4,096); 9,000: three spans, the last ragged
@pytest.mark.parametrize("N", [2, 127, 129, 4095, 4097, 9000])
def test_iterations_equal_the_host_twin(engine, N):
    st = embed_ref.random_state(N, seed=N)
    assert N < 100 or (np.diff(st[0]) == 0).any()  # some rows without an entry
    for ex, mom in ((12.0, 0.5), (1.0, 0.8)):
        got = check_iterate(engine, st, 3, ex, mom, 200.0, "N %d, exaggeration %g" % (N, ex))
        assert np.isfinite(got["y"]).all() and got["z"] > 0


def test_subnormal_coincident_and_repeated(engine):
    from scann import _hip

    rf, col, p, y, u, gain = embed_ref.random_state(300, seed=5)
    far = y.copy()
    far[17] = (1e10, -3.0)  # d = 1e20, w = 1e-20, w * w = 1e-40: below the least normal fp32
    w = np.float32(1.0) / (np.float32(1.0) + np.float32(1e10) * np.float32(1e10))
    assert 0 < w * w < np.finfo(np.float32).tiny
    got = check_iterate(engine, (rf, col, p, far, u, gain), 3, 12.0, 0.5, 200.0, "a row 1e10 away")
    assert np.isfinite(got["y"]).all()
    same = y.copy()
    same[131] = same[40]  # d = 0, w = 1 for that pair, across a block boundary
    same[41] = same[40]   # ... and within a block
    first = check_iterate(engine, (rf, col, p, same, u, gain), 3, 1.0, 0.8, 200.0, "coincident rows")
    again = engine.embed_iterate(rf, col, p, same, u, gain, 3, 1.0, 0.8, 200.0, want_grad=True)
    embed_ref.same_state(again, first, "repeat")
    plain = engine.embed_iterate(rf, col, p, same, u, gain, 3, 1.0, 0.8, 200.0)
    assert "grad" not in plain
    embed_ref.same_state(plain, first, "no grad", keys=("y", "u", "gain"))
    # a graph without any entry: repulsion only
    none = (np.zeros(301, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), y, u, gain)
    check_iterate(engine, none, 2, 12.0, 0.5, 200.0, "no edges")
    assert _hip.EMBED_MAX_ROWS == 262144


def test_six_iterations_equal_three_and_three(engine):
    st = embed_ref.random_state(4500, seed=9)  # two spans
    whole = engine.embed_iterate(*st, 6, 4.0, 0.5, 150.0, want_grad=True)
    half = engine.embed_iterate(*st, 3, 4.0, 0.5, 150.0)
    both = engine.embed_iterate(*st[:3], half["y"], half["u"], half["gain"], 3, 4.0, 0.5, 150.0, want_grad=True)
    embed_ref.same_state(both, whole, "3 + 3")


def test_no_iteration_returns_its_inputs(engine):
    st = embed_ref.random_state(200, seed=1)
    got = engine.embed_iterate(*st, 0, 12.0, 0.5, 200.0, want_grad=True)
    assert got["z"] == 0.0 and not got["grad"].any()
    for k, a in zip(("y", "u", "gain"), st[3:]):
        assert np.array_equal(got[k].view(np.uint32), a.view(np.uint32))


# ---- the fit ----

def same_fit(a, b, label):
    for k in ("coords", "neighbor_position", "neighbor_dist2"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (label, k)
    for k in ("z", "kl", "kl_init"):
        assert np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64), (label, k, a[k], b[k])
    assert a["n_edges"] == b["n_edges"] and a["learning_rate"] == b["learning_rate"]


@pytest.fixture(scope="module")
def blob_model(hip_lib):
    cfg, w, data, model = setup(n=4, local_dim=64, num_head=4, global_dim=96, dense_out=16)  # rows of 16 columns
    yield model
    model.engine.close()


def test_embed_of_the_planted_blobs(blob_model):
    from scann.models import LatentIndex
    from scann.models import latent_index as li

    rows, labels, new_rows, new_labels = embed_ref.blobs(0, new=20)
    index = LatentIndex(blob_model, "structure").add_rows(rows, ids=np.arange(600) + 1000)
    dev, emb = index.embed(perplexity=10, iterations=(100, 200))
    host, _ = index.embed(perplexity=10, iterations=(100, 200), route="host")
    same_fit(dev, host, "device against host route")
    same_fit(dev, li.embed_rows_host(rows, perplexity=10, iterations=(100, 200))[0], "device route against the all-host fit")
    share = embed_ref.blob_share(dev["coords"], labels)
    print("kl %.4f -> %.4f, share %.4f, z %.6g" % (dev["kl_init"], dev["kl"], share, dev["z"]))
    assert dev["kl"] < 0.5 * dev["kl_init"] and share >= 0.98
    assert np.array_equal(emb.ids, np.arange(600) + 1000) and (emb.atoms == -1).all() and emb.level == "structure" and emb.dim == 16
    # new rows of the same blobs, placed on the map: the nearest map row is one of their own blob
    placed = index.place(new_rows, emb)
    d = ((placed["coords"][:, None, :].astype(np.float64) - emb.coordinates[None, :, :]) ** 2).sum(axis=2)
    own = float((labels[d.argmin(axis=1)] == new_labels).mean())
    print("placed rows whose nearest map row is of their blob: %.4f" % own)
    assert own >= 0.98 and placed["coords"].shape == (120, 2) and placed["coords"].dtype == np.float32
    assert (labels[placed["nearest_position"]] == new_labels).all() and np.array_equal(placed["nearest_id"], placed["nearest_position"] + 1000)
    # the rows themselves: each is its own nearest row, at distance 0
    back = index.place(rows[:50], emb)
    assert np.array_equal(back["nearest_position"], np.arange(50)) and not back["nearest_distance"].any()
    index.free()


def check_model_fit(model, data, level, label, tmp_path):
    from scann import _hip
    from scann.models import LatentEmbedding

    n = int(np.shape(data["neighbors"])[0])
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    kw = dict(perplexity=5, iterations=(20, 30))
    got, emb = model.fit_embedding(index, **kw)
    host, _ = index.embed(route="host", **kw)
    same_fit(got, host, label)
    N = len(index)
    print("%s %s: %d rows, %d edges, kl %.4f -> %.4f" % (label, level, N, got["n_edges"], got["kl_init"], got["kl"]))
    assert got["coords"].shape == (N, 2) and np.isfinite(got["coords"]).all() and np.isfinite(got["kl"])
    ids, atoms = index.names()
    assert np.array_equal(emb.ids, ids) and np.array_equal(emb.atoms, atoms) and emb.level == level
    direct, _ = model.fit_embedding(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1, **kw)
    same_fit(direct, got, label + ", data instead of an index")
    emb.save(str(tmp_path / "emb.npz"))
    back = LatentEmbedding.load(model, str(tmp_path / "emb.npz"))
    # the same inputs placed on the map, padded and packed: each row finds itself first (or a coincident earlier row), at distance 0
    a = model.place(data, back, index, batch_size=16)
    pk = model.place(_hip.pack_inputs(data), emb, index, batch_size=16)
    y, _ = model.predict(data)
    assert np.array_equal(_bits(a["predict_property"]), _bits(y)) and np.array_equal(_bits(pk["predict_property"]), _bits(y))
    assert pk["coords"].shape == (N, 2) and np.isfinite(pk["coords"]).all() and not pk["nearest_distance"].any()
    assert (pk["nearest_position"] <= np.arange(N)).all() and np.array_equal(pk["nearest_id"], ids[pk["nearest_position"]])
    for key, fill in (("coords", 0), ("nearest_position", -1), ("nearest_id", -1), ("nearest_atom", -1), ("nearest_distance", 0)):
        want = pk[key] if level == "structure" else _hip.repad_atoms(pk[key], data["atom_mask"], fill)
        assert np.array_equal(a[key].view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), key
    index.free()


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_fit_embedding_on_the_models_rows(hip_lib, kind, level, tmp_path):
    cfg, w, data, model = setup(kind=kind, n=24 if kind == "mp2018" else 40, seed=0)
    check_model_fit(model, data, level, kind, tmp_path)


def test_fit_embedding_on_a_generic_width_handle(hip_lib, tmp_path):
    """rows of 30 and 96 columns"""
    cfg, w, data, model = setup(n=20, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    for level in ("structure", "atom"):
        check_model_fit(model, data, level, "generic", tmp_path)


def test_qm9_atom_rows_by_both_routes(hip_lib):
    """the after_Lc rows of the qm9 fixture with the default schedule's shape (exaggerated phase, then the plain one)"""
    cfg, w, data, model = setup(n=40, seed=3)
    index = model.build_index(data, level="atom", batch_size=16)
    dev, _ = index.embed(perplexity=10, iterations=(60, 120))
    host, _ = index.embed(perplexity=10, iterations=(60, 120), route="host")
    same_fit(dev, host, "qm9 after_Lc")
    print("qm9 after_Lc: %d rows, kl %.4f -> %.4f" % (len(index), dev["kl_init"], dev["kl"]))
    assert np.isfinite(dev["kl"]) and np.isfinite(dev["coords"]).all()
    index.free()


# ---- state ----

def test_nothing_else_changes(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng = u.eng
        st = embed_ref.random_state(len(u.rows[0]), seed=7)
        first = eng.embed_iterate(*st, 3, 12.0, 0.5, 200.0, want_grad=True)
        embed_ref.same_state(first, _hip.embed_iterate_host(*st, 3, 12.0, 0.5, 200.0, want_grad=True), "beside a model's index")
        u.repeat(lambda: eng.embed_iterate(*st, 3, 12.0, 0.5, 200.0, want_grad=True), lambda r: embed_ref.same_state(r, first, "repeat"), 5, 16 << 20)
    # a whole fit beside an existing index: its rows and the predictions stay
    y0, _ = model.predict(data)
    index = model.build_index(data, level="atom", batch_size=16)
    rows0 = index.rows()
    index.embed(perplexity=5, iterations=(5, 5))
    for a, b in zip(rows0, index.rows()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(_bits(model.predict(data)[0]), _bits(y0))
    index.free()


def test_training_handle(hip_lib):
    """after two training steps the iterations on the training handle equal the host twin's, and weights, gradients and the following
    (deterministic) step are those of a twin that never made the call"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    st = embed_ref.random_state(900, seed=2)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        embed_ref.same_state(eng.embed_iterate(*st, 3, 12.0, 0.5, 200.0, want_grad=True),
                             _hip.embed_iterate_host(*st, 3, 12.0, 0.5, 200.0, want_grad=True), "training handle")

    training_twin(cfg, w, pk, calls)


# ---- errors, the CLI ----

def test_errors_name_the_argument(hip_lib, monkeypatch):
    from scann import _hip
    from scann.models import LatentEmbedding, LatentIndex

    cfg, w, data, model = setup(n=4, seed=1, local_dim=64, num_head=4, global_dim=96, dense_out=16)
    eng = model.engine
    P = _hip._ptr
    rf, col, p, y, u, gain = embed_ref.random_state(20, seed=4)
    y, u, gain = y.copy(), u.copy(), gain.copy()
    before = [a.copy() for a in (y, u, gain)]
    z = C.c_double(7.0)
    grad = np.full((20, 2), 7, np.float32)

    def run(N=20, rf=rf, col=col, p=p, y=y, u=u, gain=gain, n_iter=1, ex=12.0, mom=0.5, lr=200.0, z=C.byref(z), h=eng._h):
        return eng.lib.scann_embed_iterate(h, N, P(rf), P(col), P(p), P(y), P(u), P(gain), n_iter, ex, mom, lr, z, P(grad))

    def message():
        return (eng.lib.scann_last_error(eng._h) or b"").decode()

    def changed(a, at, v):
        b = np.array(a)
        b[at] = v
        return b

    own = int(np.nonzero(np.diff(rf))[0][0])
    nan, inf = float("nan"), float("inf")
    free0, _ = eng.device_memory()
    for kw, word in ((dict(rf=None), "row_first is null"), (dict(col=None), "col is null"), (dict(p=None), "p is null"), (dict(y=None), "y is null"),
                     (dict(u=None), "u is null"), (dict(gain=None), "gain is null"), (dict(z=None), "z_out is null"), (dict(N=1), "N 1 outside 2 .. 262144"),
                     (dict(N=262145), "N 262145 outside"), (dict(rf=rf + 1), "row_first[0] = 1"), (dict(rf=changed(rf, 1, rf[-1] + 9)), "row_first decreases"),
                     (dict(col=changed(col, 3, 20)), "col[3] = 20 outside 0 .. 19"), (dict(col=changed(col, 3, -1)), "col[3] = -1 outside"),
                     (dict(col=changed(col, rf[own], own)), "is its own row"), (dict(p=changed(p, 2, -1.0)), "p[2] is negative or not finite"),
                     (dict(p=changed(p, 2, nan)), "p[2]"), (dict(y=changed(y, (5, 1), inf)), "y holds a non-finite value (row 5)"),
                     (dict(u=changed(u, (6, 0), nan)), "u holds a non-finite value (row 6)"),
                     (dict(gain=changed(gain, (0, 0), inf)), "gain holds a non-finite value (row 0)"), (dict(n_iter=-1), "n_iter -1 outside 0 .. 100000"),
                     (dict(n_iter=100001), "n_iter 100001"), (dict(ex=0.0), "exaggeration"), (dict(ex=nan), "exaggeration"), (dict(lr=-1.0), "lr"),
                     (dict(lr=inf), "lr"), (dict(mom=1.0), "momentum"), (dict(mom=-0.25), "momentum"), (dict(mom=nan), "momentum")):
        assert run(**kw) == -1 and word in message(), (word, message())
    assert eng.lib.scann_embed_iterate(None, 20, P(rf), P(col), P(p), P(y), P(u), P(gain), 1, 12.0, 0.5, 200.0, C.byref(z), None) == -1
    # nothing was written, nothing stays allocated
    assert all(np.array_equal(a, b) for a, b in zip((y, u, gain), before)) and z.value == 7.0 and np.all(grad == 7)
    assert free0 - eng.device_memory()[0] <= 8 << 20
    assert run() == 0 and z.value > 0 and not np.all(grad == 7)
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError, match="momentum"):
        eng.embed_iterate(rf, col, p, y, u, gain, 1, 12.0, 1.5, 200.0)
    with pytest.raises(ValueError, match=r"col\[3\] = 20"):
        eng.embed_iterate(rf, changed(col, 3, 20), p, y, u, gain, 1)
    rows, _ = embed_ref.blobs(1)
    index = LatentIndex(model, "structure").add_rows(rows[:50])
    for kw, word in ((dict(perplexity=1), "perplexity"), (dict(perplexity=16), "perplexity"), (dict(iterations=(5,)), "iterations"),
                     (dict(iterations=(5, -1)), "iterations"), (dict(exaggeration=0), "exaggeration"), (dict(learning_rate=0), "learning_rate"),
                     (dict(learning_rate="fast"), "learning_rate"), (dict(route="both"), "route")):
        with pytest.raises(ValueError, match=word):
            index.embed(**kw)
        with pytest.raises(ValueError, match=word):
            model.fit_embedding(index, **kw)
    monkeypatch.setattr(_hip, "EMBED_MAX_ROWS", 40)
    with pytest.raises(ValueError, match="select"):
        index.embed()
    monkeypatch.undo()
    small = LatentIndex(model, "structure").add_rows(rows[:8])
    with pytest.raises(ValueError, match="perplexity"):
        small.embed(perplexity=10)
    bad = LatentIndex(model, "structure").add_rows(changed(rows[:50], (3, 2), np.nan))
    with pytest.raises(ValueError, match="non-finite"):
        bad.embed()
    _, emb = index.embed(perplexity=5, iterations=(2, 2))
    with pytest.raises(ValueError, match="LatentEmbedding"):
        model.place(data, "a map", index)
    with pytest.raises(ValueError, match="does not map"):
        model.place(data, emb, small)
    other = LatentEmbedding(np.zeros((50, 2)), np.arange(50), np.arange(50), 5, "atom", 96)
    with pytest.raises(ValueError, match="does not map"):
        model.place(data, other, index)
    for ix in (index, small, bad):
        ix.free()


def test_cli_writes_the_embedding(hip_lib, tmp_path):
    """predict_model.py --embed writes embedding_<target>.pickle and, with --embed-out, the map; the other files' bytes are those of a run
    without the flag"""
    import yaml

    from scann.models import SCANN, LatentEmbedding
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
    r = subprocess.run(cli + ["--embed", "--embed-level", "atom", "--embed-perplexity", "5", "--embed-out", str(tmp_path / "map.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert set(os.listdir(out)) - listed == {"embedding_homo.pickle"}
    got = pickle.load(open(out / "embedding_homo.pickle", "rb"))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    want, emb = scann.fit_embedding(pool, perplexity=5)
    assert sorted(got) == sorted(list(want) + ["id", "atom"])
    same_fit(got, want, "the CLI's fit")
    assert "kl " in r.stdout and "n_rows %d" % len(pool) in r.stdout
    saved = LatentEmbedding.load(scann.model, str(tmp_path / "map.npz"))
    assert np.array_equal(saved.coordinates.view(np.uint32), emb.coordinates.view(np.uint32)) and np.array_equal(saved.ids, got["id"])
    inputs, _ = data[0]
    placed = scann.place(inputs, saved, pool)
    assert placed["coords"].shape[-1] == 2 and np.isfinite(placed["coords"]).all()
    pool.free()

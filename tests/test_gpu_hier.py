"""GPU tests of the hierarchical clustering of a latent index (scann_index_mst through Engine.index_mst; LatentIndex.hierarchy,
HipModel.hierarchy / attach).  Every comparison of a device result with the twin is an equality: edges equal, weights bit for bit.

1. The kernels == the twin scann_mst_host: N either side of the 64-row tile and of the 128-query tile, one and many workgroups and
   ranges, dim either side of the 32-column slab and no multiple of 4, the smallest and the largest widths, without and with core
   distances; lattices full of ties, coincident rows, a constant core distance, non-finite rows, distances that overflow, an empty pool.
   2. Two storage chunks.  3. One add or many; after unrelated indices were created and freed.  4. End to end on the qm9 and mp2018
   fixtures at both levels; attach behind a forward; a generic width; a training handle.  5. Errors; the CLI; the crescents."""
import math
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import hier_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import _bits, make_index, random_rows, same_arrays, setup, training_twin, untouched  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hip_lib):
    cfg, w, inputs, model = setup(n=4)
    yield model.engine
    model.engine.close()


class _Index:
    """what ``neighbour_graph`` asks of a LatentIndex, around a bare device index of any width"""

    def __init__(self, eng, ix):
        self.model, self._ix = types.SimpleNamespace(engine=eng), ix

    def __len__(self):
        return len(self._ix)


def core2_of(eng, ix, rows, min_samples=5):
    """the core distances from the device's exact search (rows without a non-finite component only)"""
    from scann.models import latent_index as li

    return li.hierarchy_core2(rows, min_samples, lambda x: li.neighbour_graph(_Index(eng, ix), strict=False))


def same_tree(got, want, label):
    assert len(got["a"]) == len(want["a"]), "%s: n_edges %d, the twin has %d" % (label, len(got["a"]), len(want["a"]))
    assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["b"], want["b"]), label + ": edges"
    assert np.array_equal(_bits(got["w"]), _bits(want["w"])), label + ": weights"


def check_pool(eng, rows, core, label):
    """the device's tree of an index of ``rows`` against the twin's; ``core``: None, an array, or an int (min_samples, from the search)"""
    from scann import _hip

    ix = make_index(eng, rows)
    try:
        if isinstance(core, int):
            core = core2_of(eng, ix, rows, core)
        got = eng.index_mst(ix, core)
    finally:
        ix.free()
    same_tree(got, _hip.mst_host(rows, core), label)
    n_el = int(np.isfinite(rows).all(axis=1).sum()) if len(rows) else 0
    assert len(got["a"]) == max(n_el - 1, 0) and (got["a"] < got["b"]).all()
    assert got["rounds"] <= (math.ceil(math.log2(n_el)) if n_el > 1 else 0), (got["rounds"], n_el)
    log = _hip.mst_last_rounds()
    print("%s: %d edges in %d rounds, components %s, tiles skipped %s of %d" % (
        label, len(got["a"]), got["rounds"], log["components"].tolist(), log["skipped"].tolist(), log["tiles"]))
    return got


# ---- 1. the kernels against the twin ----

@pytest.mark.parametrize("dim", [1, 3, 128, 130, 1024])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 5000])
def test_kernels_equal_the_host_twin(engine, N, dim):
    rows = random_rows(N, dim)
    got = check_pool(engine, rows, None, "N %d dim %d" % (N, dim))
    check_pool(engine, rows, 5, "N %d dim %d, min_samples 5" % (N, dim))
    if N >= 100:
        assert (got["w"][:4] == 0).all() and got["a"][0] == 3  # random_rows' duplicates hang on their earlier copy
    if N == 5000:
        assert got["rounds"] >= 2  # 79 ranges and 40 query tiles: merges, and later rounds with labels that repeat


def test_planted_ties_and_non_finite_rows(engine):
    rows = hier_ref.lattice_rows(700, seed=3)
    got = check_pool(engine, rows, None, "lattice")
    from scann import _hip

    k = hier_ref.kruskal(rows, None, _hip.knn_dist2_matrix)
    same_tree(got, dict(a=k[0], b=k[1], w=k[2]), "lattice against Kruskal")
    assert len(np.unique(got["w"])) <= 4
    check_pool(engine, rows, 3, "lattice, min_samples 3")
    same = np.tile(random_rows(1, 130, seed=1), (300, 1))
    got = check_pool(engine, same, None, "all coincident")
    assert (got["a"] == 0).all() and np.array_equal(got["b"], np.arange(1, 300)) and (got["w"] == 0).all() and got["rounds"] == 1
    rows = random_rows(400, 20, seed=4)
    big = np.full(400, 1e12, np.float32)
    got = check_pool(engine, rows, big, "a constant core distance")
    assert (got["a"] == 0).all() and np.array_equal(got["b"], np.arange(1, 400)) and (got["w"] == big[0]).all()
    rows = random_rows(700, 130, seed=12)
    rows[100:140] = rows[7]           # 41 coincident rows
    rows[300:364] = rows[299]         # a whole tile of them
    rows[13, 129] = np.nan
    rows[400, 128] = np.inf
    rows[401, 0] = -np.inf
    rows[401, 5] = np.nan
    rows[500] = np.float32(3e19)      # finite: every distance overflows to +inf
    rows[501] = np.float32(-3e19)
    rows[502, 64] = np.float32(1e6)   # far, not overflowing
    for core in (None, np.where(np.arange(700) % 3 == 0, 50.0, 0.0).astype(np.float32)):
        got = check_pool(engine, rows, core, "planted")
        assert not set(got["a"].tolist() + got["b"].tolist()) & {13, 400, 401} and len(got["a"]) == 696
        assert np.isinf(got["w"]).sum() == 2 and not np.isnan(got["w"]).any()
        assert list(zip(got["a"][-2:].tolist(), got["b"][-2:].tolist())) == [(0, 500), (0, 501)]  # +inf edges rank last, by position
    none = np.full((130, 5), np.nan, np.float32)
    assert len(check_pool(engine, none, None, "no eligible row")["a"]) == 0
    none[77] = 1.0
    assert len(check_pool(engine, none, None, "one eligible row")["a"]) == 0
    none[129] = 2.0
    got = check_pool(engine, none, None, "two eligible rows")
    assert (got["a"].tolist(), got["b"].tolist(), got["w"].tolist()) == ([77], [129], [5.0])


def range_geometry(N):
    """(tiles per range, workgroups of a launch) of a pass over N rows by N queries: about 4,096 workgroups, ranges of whole tiles"""
    tiles, n_qt = -(-N // 64), -(-N // 128)
    want = min(-(-4096 // n_qt), tiles, 65535)
    per = -(-tiles // want)
    return per, n_qt * -(-tiles // per)


@pytest.mark.parametrize("dim", [3, 40, 130])
def test_the_label_rule_skips_tiles_inside_a_range(engine, dim):
    """Kinds that lie together in the index, as in one built in dataset order: three well-separated blobs one after another, their
    boundaries on no tile, query-tile or range boundary, at a size where a range holds 18 tiles.  Once a blob is one component, the
    workgroups whose queries lie inside it skip its tiles: at the start, in the middle and at the end of a range, several in a row,
    with one slab per tile (dim 3) and with more (dim 40: 2, dim 130: 5; the next tile's first slab is in flight).  The middle blob's
    rows coincide, so it is one component after round 1 whatever the other two do, and the rule fires from round 2 on.  The tree is
    the twin's, without and with core distances, and more tiles were skipped in one round than the launch has workgroups: some
    workgroup skipped several."""
    from scann import _hip

    sizes = (8100, 7870, 8030)
    N = sum(sizes)
    per, n_wg = range_geometry(N)
    assert per >= 4, per  # several tiles per range
    rng = np.random.default_rng(dim)
    centres = np.zeros((3, dim), np.float32)
    centres[1, 0], centres[2, min(1, dim - 1)] = 200.0, -300.0
    rows = (centres[np.repeat(np.arange(3), sizes)] + rng.standard_normal((N, dim))).astype(np.float32)
    rows[sizes[0]:sizes[0] + sizes[1]] = centres[1]  # the middle blob: one point, a star under row 8100 after round 1
    rows[5000] = rows[4999]  # a tie inside a blob
    for core in (None, 5):
        got = check_pool(engine, rows, core, "three blobs in position order, dim %d" % dim)
        log = _hip.mst_last_rounds()
        assert log["tiles"] == -(-N // 64) * -(-N // 128) and log["skipped"][0] == 0  # round 1: every row is a component of its own
        assert log["skipped"][1] > n_wg, (log["skipped"].tolist(), n_wg)  # the middle blob alone: about 61 query tiles x 122 tiles
        assert log["skipped"].max() <= log["tiles"] and (np.diff(log["skipped"]) >= 0).all()  # components only grow
        # the two last edges join the blobs
        blob = np.repeat(np.arange(3), sizes)
        assert (blob[got["a"][:-2]] == blob[got["b"][:-2]]).all() and (blob[got["a"][-2:]] != blob[got["b"][-2:]]).all()


def test_hierarchy_of_an_index_with_non_finite_rows(hip_lib):
    """LatentIndex.hierarchy on the device with rows that do not count: the core distances come from a search over the other rows in
    a temporary index -- the host route's and hierarchy_rows_host's bits"""
    from scann.models import LatentIndex
    from scann.models import latent_index as li

    cfg, w, data, model = setup(n=4)
    rows = random_rows(600, 128, seed=21)
    rows[0, 5] = np.nan
    rows[77] = np.inf
    rows[599, 127] = -np.inf
    index = LatentIndex(model, "structure").add_rows(rows[:300]).add_rows(rows[300:])
    free0, _ = model.engine.device_memory()
    for ms in (5, 0):
        res, h = index.hierarchy(min_samples=ms)
        want, _ = li.hierarchy_rows_host(rows, min_samples=ms)
        same_tree(res, want, "non-finite rows, min_samples %d" % ms)
        assert res["n_eligible"] == 597 and len(res["a"]) == 596 and h.cut(k=2)[[0, 77, 599]].tolist() == [-1, -1, -1]
        if ms:
            assert np.array_equal(_bits(res["core2"]), _bits(want["core2"])) and (res["core2"][[0, 77, 599]] == 0).all() and (res["core2"][1:77] > 0).all()
        host, _ = index.hierarchy(min_samples=ms, route="host")
        same_tree(host, want, "the host route")
    assert free0 - model.engine.device_memory()[0] <= 16 << 20  # the temporary index went back
    lone = LatentIndex(model, "structure").add_rows(np.where(np.arange(5)[:, None] == 3, rows[:5], np.nan).astype(np.float32))
    res, h = lone.hierarchy(min_samples=5)
    assert len(res["a"]) == 0 and res["n_eligible"] == 1 and h.cut(k=1).tolist() == [-1, -1, -1, 0, -1] and res["rounds"] == 0
    index.free()
    lone.free()
    model.engine.close()


def test_an_empty_pool(engine):
    ix = engine.index_create(8)
    try:
        r = engine.index_mst(ix)
        assert r["a"].shape == (0,) and r["b"].shape == (0,) and r["w"].shape == (0,) and r["rounds"] == 0
    finally:
        ix.free()


# ---- 2. two storage chunks ----

def test_tree_over_two_chunks(engine):
    """17,000 x 1,024: a storage chunk holds 16,384 rows of 1,024 columns; query tiles and row ranges both cross the boundary"""
    rows = random_rows(17000, 1024)
    got = check_pool(engine, rows, None, "17,000 x 1,024")
    across = (got["a"] < 16384) & (got["b"] >= 16384)
    assert across.any() and (got["b"] < 16384).any() and (got["a"] >= 16384).any()


# ---- 3. invariance ----

def test_results_do_not_depend_on_how_the_pool_was_built(engine):
    dim, N = 130, 3000
    rows = random_rows(N, dim, seed=9)
    one = make_index(engine, rows)
    core = core2_of(engine, one, rows, 5)
    first = engine.index_mst(one, None), engine.index_mst(one, core)
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
        for c, want in zip((None, core), first):
            same_tree(engine.index_mst(many, c), want, "many adds")
            same_tree(engine.index_mst(one, c), want, "repeat")
    finally:
        junk[1].free()
        one.free()
        many.free()


# ---- 4. end to end ----

E2E = {"qm9": 40, "mp2018": 24}


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


def attach_rule(rows, pool_rows, h, clusters):
    """the attach rule evaluated on the host: (label, nearest position, dist2) of every row"""
    from scann import _hip

    d = _hip.knn_dist2_matrix(rows, pool_rows)
    pos = np.argmin(d, axis=1)  # (the first among equal distances: the search's order)
    d2 = d[np.arange(len(rows)), pos]
    label = []
    for p, x in zip(pos.tolist(), d2.tolist()):
        lab = int(clusters["label"][p])
        if lab >= 0 and max(np.float32(x), h.core2[p]) >= clusters["birth2"][lab]:
            lab = -1
        label.append(lab)
    return np.array(label, np.int32), pos.astype(np.int32), d2


def check_attach(model, data, level, label, min_samples=3, mcs=4):
    """attach of ``data`` under the hierarchy of every second structure's rows: y, ga a plain predict's; labels the host rule's"""
    from scann import _hip

    n = int(np.shape(data["neighbors"])[0])
    half = {k: np.asarray(v)[::2] for k, v in data.items()}
    index = model.build_index(half, level=level, batch_size=16)
    res, h = model.hierarchy(index, min_samples=min_samples, min_cluster_size=mcs)
    clusters = h.clusters(mcs)
    assert np.array_equal(res["label"], clusters["label"])
    got = model.attach(data, h, index, mcs, batch_size=16)
    y, ga = model.predict(data)
    assert np.array_equal(_bits(got["predict_property"]), _bits(y)) and np.array_equal(_bits(got["global_attention"]), _bits(ga)), label
    pk = _hip.pack_inputs(data)
    rb = model.engine.upload(pk)
    _, _, level_rows = level_rows_of(model.engine, rb)
    rb.free()
    want, pos, d2 = attach_rule(level_rows[level], index.rows()[0], h, clusters)
    packed = model.attach(pk, h, index, mcs, batch_size=16)
    assert np.array_equal(packed["label"], want) and np.array_equal(packed["nearest_position"], pos), label
    assert np.array_equal(_bits(packed["nearest_distance"]), _bits(np.sqrt(d2))) and np.array_equal(_bits(packed["predict_property"][:, 0]), _bits(y[:, 0]))
    if level == "atom":
        assert np.array_equal(got["label"], _hip.repad_atoms(want, data["atom_mask"], -1))
    else:
        assert np.array_equal(got["label"], want)
    print("%s %s: %d clusters over %d rows; %d of %d new rows attached" % (label, level, len(clusters["size"]), len(index), int((want >= 0).sum()), len(want)))
    assert n and packed["label"].dtype == np.int32
    index.free()
    return h


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_hierarchy_of_a_model_is_the_twin_on_its_rows(hip_lib, kind, level, tmp_path):
    from scann.models import LatentHierarchy
    from scann.models import latent_index as li

    n = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n, seed=0)
    index = model.build_index(data, level=level, batch_size=16, ids=np.arange(n) * 2 + 1)
    rows, ids, atoms = index.rows()
    for ms in (5, 0):
        res, h = model.hierarchy(index, min_samples=ms, min_cluster_size=4)
        want, h_w = li.hierarchy_rows_host(rows, min_samples=ms, ids=ids, atoms=atoms, level=level)
        same_tree(res, want, "%s %s min_samples %d" % (kind, level, ms))
        assert res["n_eligible"] == len(rows) and 1 <= res["rounds"] <= math.ceil(math.log2(len(rows)))
        if ms:
            assert np.array_equal(_bits(res["core2"]), _bits(want["core2"]))
        c = h_w.clusters(4)
        for key in ("label", "exemplar", "size"):
            assert np.array_equal(res[key], c[key]), key
        for key in ("probability", "persistence"):
            assert np.array_equal(res[key].view(np.uint64), c[key].view(np.uint64)), key
        host, _ = index.hierarchy(min_samples=ms, route="host")
        same_tree(host, want, "the host route")
        print("%s %s min_samples %d: %d rows, %d rounds, %d clusters, %d noise" % (
            kind, level, ms, len(rows), res["rounds"], len(res["size"]), int((res["label"] < 0).sum())))
    assert np.array_equal(h.ids, ids) and np.array_equal(h.atoms, atoms) and h.level == level
    direct, _ = model.hierarchy(data, level=level, min_samples=0, batch_size=16, ids=np.arange(n) * 2 + 1)
    same_tree(direct, res, "data instead of an index")
    assert "label" not in direct
    h.save(str(tmp_path / "h.npz"))
    back = LatentHierarchy.load(model, str(tmp_path / "h.npz"))
    assert np.array_equal(back.cut(k=3), h.cut(k=3)) and np.array_equal(back.linkage(), h.linkage())
    index.free()
    check_attach(model, data, level, kind)


def test_generic_width_handle(hip_lib):
    """rows of 30 and 96 columns, the first no multiple of 4"""
    from scann import _hip

    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    for level in ("structure", "atom"):
        index = model.build_index(data, level=level)
        res, h = model.hierarchy(index, min_samples=2)
        same_tree(res, _hip.mst_host(index.rows()[0], res["core2"]), "generic width, " + level)
        index.free()
        check_attach(model, data, level, "generic", min_samples=2, mcs=2)


def test_nothing_else_changes(hip_lib):
    cfg, w, data, model = setup(n=40, seed=2)
    with untouched(model, data) as u:
        eng, pool = u.eng, u.pool
        core = core2_of(eng, pool, u.rows[0], 4)
        first = eng.index_mst(pool, core)
        u.repeat(lambda: eng.index_mst(pool, core), lambda r: same_tree(r, first, "repeat"), 5, 16 << 20)


def test_training_handle(hip_lib):
    """after two training steps the tree and attach's search on the training handle equal the twin's and an inference handle's, and
    weights, gradients and the following (deterministic) step -- the Adam state entered it -- are those of a handle that never made the
    calls"""
    from scann import _hip

    cfg, w, data, _ = setup(n=8, seed=5, n_attention=2)
    pk = _hip.pack_inputs(data)
    rows = random_rows(900, 128, seed=8)

    def calls(train_model, rb, inference):
        eng = train_model.engine
        ix = make_index(eng, rows)
        core = core2_of(eng, ix, rows, 5)
        want = _hip.mst_host(rows, core)
        same_tree(eng.index_mst(ix, core), want, "training handle")
        inf_model, rb2 = inference()
        inf = inf_model.engine
        ix2 = make_index(inf, rows)
        same_tree(inf.index_mst(ix2, core), want, "inference handle")
        for level in (_hip.OUT_BF_PROPERTY, _hip.OUT_AFTER_LC):  # attach's device call, k = 1
            db = [e.index_query_batch(x, b, level, 1) for e, x, b in ((eng, ix, rb), (inf, ix2, rb2))]
            same_arrays(db[0], db[1], "training against inference handle")
        ix.free()
        ix2.free()
        # HipModel.attach itself on the training handle: the inference model's answer, and the rule's labels
        from scann.models import LatentIndex
        from scann.models import latent_index as li

        _, _, level_rows = level_rows_of(inf, rb2)
        pool_rows = np.concatenate([level_rows["atom"][::2], rows[:200]])
        _, h = li.hierarchy_rows_host(pool_rows, min_samples=3, level="atom")
        att = []
        for m_ in (train_model, inf_model):
            lat = LatentIndex(m_, "atom").add_rows(pool_rows)
            att.append(m_.attach(pk, h, lat, 4))
            lat.free()
        same_arrays(att[0], att[1], "attach on the training handle")
        want_label, want_pos, _ = attach_rule(level_rows["atom"], pool_rows, h, h.clusters(4))
        assert np.array_equal(att[0]["label"], want_label) and np.array_equal(att[0]["nearest_position"], want_pos)
        assert (att[0]["nearest_distance"][::2] == 0).all()

    training_twin(cfg, w, pk, calls)


# ---- 5. errors, the CLI, the crescents ----

def test_errors_name_what_is_wrong(hip_lib):
    from scann import _hip
    from scann.models import LatentHierarchy

    cfg, w, data, model = setup(n=4, seed=1)
    eng = model.engine
    cfg2, w2, _, other = setup(n=4, seed=1)
    rows = random_rows(5, 4, seed=0)
    pool, foreign = make_index(eng, rows), make_index(other.engine, rows)
    P = _hip._ptr
    ne, a, b, wt, rounds = np.full(1, 7, np.int64), np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7, np.float32), np.full(1, 7, np.int32)
    nan, neg = np.zeros(5, np.float32), np.zeros(5, np.float32)
    nan[2], neg[4] = np.nan, -0.5

    def message():
        return (eng.lib.scann_last_error(eng._h) or b"").decode()

    def mst(p=pool, core=None, ne=ne, a=a, b=b, w=wt):
        return eng.lib.scann_index_mst(eng._h, None if p is None else p._h, P(core), P(ne), P(a), P(b), P(w), P(rounds))

    free0, _ = eng.device_memory()
    assert mst(p=None) == -1 and "scann_index_mst: null handle or pool" in message()
    assert mst(p=foreign) == -1 and "pool belongs to another handle" in message()
    assert mst(ne=None) == -1 and "n_edges is null" in message()
    assert mst(a=None) == -1 and "a is null" in message()
    assert mst(b=None) == -1 and "b is null" in message()
    assert mst(w=None) == -1 and "w is null" in message()
    assert mst(core=nan) == -1 and "core2[2] is NaN" in message()
    assert mst(core=neg) == -1 and "core2[4] is negative" in message()
    big = make_index(eng, np.zeros((_hip.MST_MAX_ROWS + 1, 1), np.float32))  # one row too many: refused before any launch
    free0, _ = eng.device_memory()
    assert mst(p=big) == -2 and "262145 rows, above SCANN_MST_MAX_ROWS = 262144" in message()
    with pytest.raises(_hip.ScannHipError, match="SCANN_MST_MAX_ROWS"):
        eng.index_mst(big)
    # nothing was written, nothing stays allocated
    assert ne[0] == 7 and (a == 7).all() and (b == 7).all() and (wt == 7).all() and rounds[0] == 7 and free0 - eng.device_memory()[0] <= 8 << 20
    assert mst() == 0 and ne[0] == 4 and 1 <= rounds[0] <= 3 and (a < b).all()
    # the Python layers: ValueError before any device call
    with pytest.raises(ValueError, match=r"core2\[2\] is NaN"):
        eng.index_mst(pool, nan)
    with pytest.raises(ValueError, match="one value per row"):
        eng.index_mst(pool, np.zeros(4, np.float32))
    lat = model.build_index(data)
    for kw, word in ((dict(min_samples=-1), "min_samples"), (dict(min_samples=32), "min_samples"), (dict(route="gpu"), "route")):
        with pytest.raises(ValueError, match=word):
            lat.hierarchy(**kw)
    with pytest.raises(ValueError, match="min_cluster_size"):
        model.hierarchy(lat, min_cluster_size=1)
    with pytest.raises(ValueError):
        other.hierarchy(lat)  # another model's index
    with pytest.raises(ValueError, match="level"):
        model.hierarchy(data, level="bond")
    _, h = model.hierarchy(lat, min_samples=1)
    with pytest.raises(ValueError, match="LatentHierarchy"):
        model.attach(data, "a tree", lat, 2)
    with pytest.raises(ValueError, match="LatentIndex"):
        model.attach(data, h, "an index", 2)
    with pytest.raises(ValueError, match="min_cluster_size"):
        model.attach(data, h, lat, 1)
    with pytest.raises(ValueError, match="not built on this index"):
        model.attach(data, LatentHierarchy([], [], [], None, 1, [0], [0], 0, "structure", h.dim), lat, 2)
    for ix in (pool, foreign, lat, big):
        ix.free()


def test_cli_writes_and_loads_a_tree(hip_lib, tmp_path):
    """predict_model.py --hierarchy writes hierarchy_<target>.pickle and, with --hierarchy-out, the tree and its index, which load back;
    --attach pickles the labels under them"""
    import yaml

    from scann.models import SCANN, LatentHierarchy, LatentIndex
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
    tree = str(tmp_path / "tree.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict_model.py"), str(out), "--hierarchy", "4", "--hierarchy-min-samples", "3",
                        "--hierarchy-out", tree, "--attach", tree, "--attach-min-cluster-size", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert {"hierarchy_homo.pickle", "attach_homo.pickle"} <= set(os.listdir(out))
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="atom", ids=data.indexes)
    want, h = scann.hierarchy(pool, min_samples=3, min_cluster_size=4)
    got = pickle.load(open(out / "hierarchy_homo.pickle", "rb"))
    assert sorted(got) == sorted(list(want) + ["id", "atom"])
    for key in ("a", "b", "label", "exemplar", "size"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(_bits(got["w"]), _bits(want["w"])) and "rounds" in r.stdout and "noise" in r.stdout
    saved = LatentHierarchy.load(scann.model, tree)
    assert np.array_equal(saved.a, h.a) and np.array_equal(_bits(saved.core2), _bits(h.core2)) and np.array_equal(saved.ids, h.ids) and saved.min_samples == 3
    index = LatentIndex.load(scann.model, tree + ".index.npz")
    assert np.array_equal(_bits(index.rows()[0]), _bits(pool.rows()[0]))
    per = pickle.load(open(out / "attach_homo.pickle", "rb"))
    inputs, _ = data[0]
    first = scann.attach(inputs, saved, index, 4)
    amask = np.asarray(inputs["atom_mask"]).reshape(np.shape(inputs["neighbors"])[:2]) != 0
    assert len(per) == n and sorted(per[0]) == ["label", "nearest_atom", "nearest_distance", "nearest_id", "predict_property"]
    assert np.array_equal(per[0]["label"], first["label"][0][amask[0]]) and (per[0]["nearest_distance"] >= 0).all()
    pool.free()
    index.free()


@pytest.mark.parametrize("min_samples,min_cluster_size", [(5, 20), (10, 50)])
def test_crescents_with_outliers_on_the_device(engine, min_samples, min_cluster_size):
    """800 of 800 rows in their crescent, 80 of 80 outliers noise, from the device's tree"""
    from scann.models import LatentHierarchy

    rows, planted = hier_ref.crescents_with_outliers(0)
    ix = make_index(engine, rows)
    try:
        core = core2_of(engine, ix, rows, min_samples)
        got = engine.index_mst(ix, core)
    finally:
        ix.free()
    h = LatentHierarchy(got["a"], got["b"], got["w"], core, len(rows), np.arange(len(rows)), np.full(len(rows), -1), min_samples, "structure", 16)
    c = h.clusters(min_cluster_size)
    real = planted >= 0
    assert len(c["size"]) == 2 and (c["label"][~real] == -1).all(), "%d of 80 outliers are noise" % int((c["label"][~real] == -1).sum())
    assert (c["label"][real] >= 0).all() and hier_ref.same_partition(c["label"][real], planted[real])

"""GPU tests of an index's partition into cells and of the nearest-row search that skips cells out of reach (scann_index_partition,
scann_index_search_stats, scann_index_query_rows through Engine.index_*, LatentIndex.partition, HipModel.build_index(cells=...)).

Every comparison is bitwise; on a mismatch the query, the place and both (dist2, position) pairs are printed.
1. Exactness: two indices of the same rows, one partitioned -- index_query gives equal bytes on both, and both equal the total-order
   selection (tests/knn_ref.py) over the host twin's distances.  Sizes round the tile (63, 64, 65), several groups of queries, cells > N, an
   index of two storage chunks; integer grids where hundreds of distances tie across cells; the planted cases of tests/test_gpu_knn.py;
   query ids; non-finite rows and queries.
2. The partition on the device equals the host twin (and so the definition, tests/test_cells_host.py) in every byte; add and
   partition(0) drop it.
3. Skipping happens: on 8 well-separated blobs at most half of the (group, tile) pairs are visited -- the assertion the NumPy pruned
   search of tests/test_cells_host.py passes on the CPU.
4. Downstream: index_query_rows, the neighbour graph, index_select against a partitioned reference, HipModel.nearest / place / attach;
   the analyses that never read the copy; save / load; selected outputs and training state; errors.
5. The fall-back to the full kernel where the plan keeps more than half of a pass's pairs at k <= 3: bytes and stats."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import cells_ref  # noqa: E402
import knn_ref  # noqa: E402
import scann_oracle as so  # noqa: E402
from analysis_checks import _bits  # noqa: E402
from test_cells_host import blobs  # noqa: E402

pytestmark = pytest.mark.gpu


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_dict(a, b, label):
    assert sorted(a) == sorted(b), label
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert _bytes_equal(a[key], b[key]), (label, key)
        else:
            assert a[key] == b[key], (label, key)


def setup(n=24, seed=0):
    from scann.models.scann_model import HipModel

    cfg = so.default_config("qm9")
    w = so.init_weights(cfg, 1234, perturb=True)
    inputs, _ = so.pad_batch(*so.synth_dataset(n, seed, kind="qm9"), g_update=cfg["model"]["g_update"])
    return cfg, w, {k: np.array(v) for k, v in inputs.items()}, HipModel(cfg, w, device=0, infer=True)


@pytest.fixture(scope="module")
def model(hip_lib):
    cfg, w, inputs, m = setup(n=24)
    m.inputs24 = inputs
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def engine(model):
    return model.engine


class Pair:
    """the same rows in two indices, the second one partitioned"""

    def __init__(self, eng, rows, cells, ids=None, atoms=None, max_iter=4):
        self.eng, self.rows = eng, np.ascontiguousarray(rows, np.float32)
        n = len(rows)
        self.ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.atoms = np.full(n, -1, np.int32) if atoms is None else np.asarray(atoms, np.int32)
        self.plain, self.cut = eng.index_create(rows.shape[1]), eng.index_create(rows.shape[1])
        for ix in (self.plain, self.cut):
            eng.index_add(ix, self.rows, self.ids, self.atoms)
        self.info = eng.index_partition(self.cut, cells, max_iter)

    def free(self):
        self.plain.free()
        self.cut.free()

    def check(self, q, k, label, query_ids=None):
        """index_query on both indices and the total-order selection over the host distances: all equal in every byte"""
        from scann import _hip

        q = np.ascontiguousarray(q, np.float32)
        a = self.eng.index_query(self.plain, q, k, query_ids=query_ids)
        st_plain = self.eng.index_search_stats(self.plain)
        b = self.eng.index_query(self.cut, q, k, query_ids=query_ids)
        st = self.eng.index_search_stats(self.cut)
        with np.errstate(all="ignore"):
            d = _hip.knn_dist2_matrix(q, self.rows)
        od, op, oi, oa = knn_ref.select(d, k, ids=self.ids, atoms=self.atoms, query_ids=query_ids)
        print("%s: N %d, dim %d, Q %d, k %d, cells %d: visited %d of %d pairs (%d seeds, %d groups)" % (
            label, len(self.rows), q.shape[1], len(q), k, self.info["cells"], st["visited"], st["total"], st["seeds"], st["groups"]))
        for name, got in (("partitioned", b), ("full", a)):
            wrong = np.argwhere((got["position"] != op) | (_bits(got["dist2"]) != _bits(od)))
            for i, j in wrong[:8]:
                print("  %s index, query %d, place %d: got (%r, %d), the selection has (%r, %d)" % (
                    name, i, j, got["dist2"][i, j], got["position"][i, j], od[i, j], op[i, j]))
            assert len(wrong) == 0, (label, name, len(wrong))
            assert np.array_equal(got["id"], oi) and np.array_equal(got["atom"], oa), (label, name)
        same_dict(a, b, label)
        groups = -(-len(q) // 128) if len(q) <= 1024 else None
        assert st_plain["visited"] == st_plain["total"] and st_plain["seeds"] == 0 and st["total"] == st_plain["total"]
        assert groups is None or st["groups"] == st_plain["groups"] == groups
        assert 0 <= st["seeds"] <= st["visited"]
        return b, st


def clustered(rng, n, dim, spread=8.0, kinds=5):
    return (rng.standard_normal((n, dim)) + rng.integers(0, kinds, (n, 1)) * spread * rng.standard_normal((1, dim))).astype(np.float32)


# N, dim, cells, k, Q: N in {1, 63, 64, 65, 130, 1,000, 5,000}, dim in {1, 2, 33, 128, 130}, cells in {1, 2, 7, 64} and cells > N,
# k in {1, 5, 32}, Q in {1, 7, 128, 129, 300}; and one index of 1,024 columns and 17,000 rows that spans two storage chunks
EXACT_CASES = [(1, 1, 1, 1, 1), (1, 128, 7, 5, 7), (63, 2, 2, 32, 129), (63, 33, 64, 5, 1), (64, 128, 1, 32, 7), (64, 2, 7, 1, 128),
               (65, 130, 2, 5, 129), (65, 1, 64, 32, 300), (130, 33, 7, 32, 128), (130, 2, 200, 5, 7), (1000, 128, 64, 5, 300),
               (1000, 1, 7, 32, 129), (1000, 130, 2, 1, 128), (5000, 128, 64, 32, 129), (5000, 33, 7, 5, 300), (5000, 2, 64, 1, 1),
               (17000, 1024, 7, 5, 7)]


@pytest.mark.parametrize("N,dim,cells,k,Q", EXACT_CASES, ids=["N%d_d%d_c%d_k%d_Q%d" % c for c in EXACT_CASES])
def test_pruned_search_is_exact(engine, N, dim, cells, k, Q):
    rng = np.random.default_rng(N * 7 + dim * 3 + cells + k + Q)
    rows = clustered(rng, N, dim)
    ids = rng.integers(0, 1 << 40, N).astype(np.int64)
    atoms = rng.integers(-1, 30, N).astype(np.int32)
    q = np.concatenate([rows[rng.integers(0, N, Q - Q // 2)] + np.float32(0.05) * rng.standard_normal((Q - Q // 2, dim)).astype(np.float32),
                        clustered(rng, Q // 2, dim)]).astype(np.float32)
    p = Pair(engine, rows, cells, ids, atoms)
    try:
        assert p.info["cells"] == min(cells, N) and p.info["tiles"] * 64 - p.info["pad"] == N
        p.check(q, k, "clustered")
        if N >= 63 and Q >= 7:  # leave-one-out against ids that occur in the index
            p.check(q, k, "clustered, exclude", query_ids=ids[rng.integers(0, N, Q)])
    finally:
        p.free()


def test_ties_across_cells(engine):
    rng = np.random.default_rng(2)
    grid = rng.integers(0, 4, (900, 2)).astype(np.float32)
    p = Pair(engine, grid, 7)
    try:
        got, _ = p.check(rng.integers(0, 4, (129, 2)).astype(np.float32), 32, "grid {0..3}^2")
        assert (np.diff(got["dist2"], axis=1) == 0).sum() > 1000  # hundreds of exact ties, resolved by position
    finally:
        p.free()
    cube = np.zeros((700, 128), np.float32)
    cube[:, :8] = rng.integers(0, 2, (700, 8))
    qc = np.zeros((129, 128), np.float32)
    qc[:, :8] = rng.integers(0, 2, (129, 8))
    p = Pair(engine, cube, 9)
    try:
        got, _ = p.check(qc, 32, "cube {0,1}^8 in 128 columns")
        assert (np.diff(got["dist2"], axis=1) == 0).sum() > 1000
    finally:
        p.free()


def test_planted_cases(engine):
    rng = np.random.default_rng(5)
    dim, N = 128, 1000
    rows = (rng.standard_normal((N, dim)) * 3).astype(np.float32)
    q = (rng.standard_normal((16, dim)) * 3).astype(np.float32)
    rows[700] = q[0] + np.float32(0.25)  # exact duplicates of one row near query 0, at positions out of order
    rows[[20, 350, 999]] = rows[700]
    rows[[640, 64]] = q[1]  # query 1 itself, twice
    near = 100 + 63 * np.arange(8)  # near-duplicates of queries 2 .. 9 among far rows
    rows[near] = q[2:10] + np.float32(1e-3) * rng.standard_normal((8, dim)).astype(np.float32)
    ids = np.arange(N, dtype=np.int64) + 5000
    atoms = (np.arange(N) % 17).astype(np.int32)
    for cells in (1, 7, 64):
        p = Pair(engine, rows, cells, ids, atoms)
        try:
            got, _ = p.check(q, 5, "planted, %d cells" % cells)
            assert np.array_equal(got["position"][0, :4], [20, 350, 700, 999]) and len(set(got["dist2"][0, :4])) == 1
            assert np.array_equal(got["position"][1, :2], [64, 640]) and not got["dist2"][1, :2].any() and got["dist2"][1, 2] > 0
            assert np.array_equal(got["position"][2:10, 0], near)
            p.check(q, 5, "planted, exclude", query_ids=np.array([5020, 5064] + [0] * 14, dtype=np.int64))
        finally:
            p.free()


def test_query_ids_and_k_beyond_the_rows(engine):
    rng = np.random.default_rng(8)
    rows = clustered(rng, 300, 33)
    ids = (np.arange(300) // 75).astype(np.int64)  # four segments
    q = rows[rng.integers(0, 300, 40)] + np.float32(0.01)
    p = Pair(engine, rows, 7, ids)
    try:
        p.check(q, 5, "a whole segment excluded", query_ids=np.full(40, 1, np.int64))
        p.check(q, 32, "k = 32")
    finally:
        p.free()
    p = Pair(engine, rows[:20], 4, np.zeros(20, np.int64))
    try:
        got, _ = p.check(q, 32, "k > N")
        assert np.all(got["position"][:, 20:] == -1) and np.all(np.isinf(got["dist2"][:, 20:])) and np.all(got["position"][:, :20] >= 0)
        got, _ = p.check(q, 5, "every row excluded", query_ids=np.zeros(40, np.int64))
        assert np.all(got["position"] == -1) and np.all(got["id"] == -1) and np.all(np.isinf(got["dist2"]))
    finally:
        p.free()


def test_non_finite_rows_and_queries(engine):
    rng = np.random.default_rng(9)
    rows = clustered(rng, 400, 33)
    rows[[3, 200]] = np.nan
    rows[77, 5] = np.inf
    rows[[150, 151]] = np.float32(3e19)  # finite rows whose distances overflow to +inf
    q = rows[rng.integers(0, 400, 60)] + np.float32(0.01)
    q[4, 0] = np.nan
    q[9] = np.float32(3e19)
    p = Pair(engine, rows, 7)
    try:
        for k in (1, 32):
            got, _ = p.check(q, k, "non-finite")
            assert np.all(got["position"][4] == -1)  # every distance of a NaN query is NaN
        cells = engine.index_cells_read(p.cut)
        loose = cells["perm"][64 * cells["first_tile"][cells["cells"]]:]
        assert np.array_equal(loose[loose >= 0], [3, 77, 200])
    finally:
        p.free()


# ---- the partition on the device ----

TWIN_CASES = [(1, 3, 1), (63, 2, 64), (64, 33, 7), (65, 3, 4), (1000, 5, 5), (1000, 2, 64)]


@pytest.mark.parametrize("n,dim,cells", TWIN_CASES, ids=["N%d_d%d_c%d" % c for c in TWIN_CASES])
def test_device_partition_equals_the_host_twin(engine, n, dim, cells):
    from scann import _hip
    from test_cells_host import _case_rows

    for name in ("random", "blobs", "identical", "nonfinite", "grid"):
        rows = _case_rows(name, n, dim, np.random.default_rng(n + cells))
        ix = engine.index_create(dim)
        try:
            engine.index_add(ix, rows)
            info = engine.index_partition(ix, cells, 4)
            got, want = engine.index_cells_read(ix), _hip.cells_host(rows, cells, 4)
            cells_ref.same(got, want, name)
            assert info == {key: want[key] for key in _hip.CELLS_INFO} and engine.index_partition_args(ix) == (cells, 4)
        finally:
            ix.free()


def test_add_and_cells_0_drop_the_partition(engine):
    rng = np.random.default_rng(4)
    rows = clustered(rng, 500, 33)
    q = rows[:50] + np.float32(0.01)
    p = Pair(engine, rows, 7)
    try:
        assert engine.index_cells_read(p.cut)["cells"] == 7
        more = clustered(rng, 70, 33)
        for ix in (p.plain, p.cut):
            engine.index_add(ix, more, np.arange(70, dtype=np.int64) + 500, np.full(70, -1, np.int32))
        p.rows, p.ids, p.atoms = np.concatenate([rows, more]), np.arange(570, dtype=np.int64), np.full(570, -1, np.int32)
        assert engine.index_cells_read(p.cut)["cells"] == 0 and engine.index_partition_args(p.cut) == (0, 0)
        a = engine.index_query(p.cut, q, 5)
        st = engine.index_search_stats(p.cut)
        assert st["visited"] == st["total"] == 9 and st["seeds"] == 0  # 570 rows: 9 tiles, one group
        same_dict(a, engine.index_query(p.plain, q, 5), "after add")
        p.info = engine.index_partition(p.cut, 7)
        p.check(q, 5, "partitioned again")
        assert engine.index_partition(p.cut, 0) == {"cells": 0, "tiles": 0, "pad": 0, "largest": 0}
        assert engine.index_cells_read(p.cut)["tiles"] == 0
        engine.index_query(p.cut, q, 5)
        st = engine.index_search_stats(p.cut)
        assert st["visited"] == st["total"]
    finally:
        p.free()
    empty = engine.index_create(8)
    try:
        assert engine.index_partition(empty, 4)["tiles"] == 0 and engine.index_cells_read(empty)["cells"] == 0
    finally:
        empty.free()


# ---- skipping must actually happen ----

def test_blobs_visit_at_most_half(engine):
    rows, q = blobs()
    p = Pair(engine, rows, 8)
    try:
        _, st = p.check(q, 5, "blobs")
        assert st["groups"] == 2 and st["total"] == 2 * 64
        assert 2 * st["visited"] <= st["total"], st
    finally:
        p.free()


def test_unstructured_rows_stay_exact_and_fall_back_at_small_k(engine):
    """Gaussian rows prune nothing.  At k = 32 the list route answers (every tile of the copy visited once); at k <= 3 a pass whose plan
    keeps more than half of its pairs goes to the full kernel, and the stats say so: visited = total + seeds.  Blobs at the same k do
    not fall back (test_blobs_visit_at_most_half)."""
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((2000, 128)).astype(np.float32)
    q = rng.standard_normal((129, 128)).astype(np.float32)
    p = Pair(engine, rows, 16)
    try:
        _, st = p.check(q, 32, "gaussian, k = 32")
        assert st["total"] < st["visited"] <= 2 * p.info["tiles"] < st["total"] + st["seeds"], st  # (no more than every tile of the copy, once)
        _, st = p.check(q, 4, "gaussian, k = 4")  # (k <= 7 falls back on a copy of 16,384 tiles or more only: not a test's size)
        assert st["total"] < st["visited"] <= 2 * p.info["tiles"] < st["total"] + st["seeds"], st
        for k in (1, 3):
            _, st = p.check(q, k, "gaussian, k = %d" % k)
            assert st["seeds"] > 0 and st["visited"] == st["total"] + st["seeds"] and st["groups"] == 2, st
            _, st = p.check(q, k, "gaussian, exclude, k = %d" % k, query_ids=np.arange(129, dtype=np.int64))
            assert st["visited"] == st["total"] + st["seeds"], st
        # more than one pass, the queries of the second one fewer than a group: each pass decides for itself
        both = np.concatenate([q, rows[:1000] + np.float32(0.01)]).astype(np.float32)
        _, st = p.check(both, 2, "gaussian, two passes")
        assert st["groups"] == 8 + 1 and st["visited"] == st["total"] + st["seeds"], st
    finally:
        p.free()


def test_fall_back_reaches_k_7_on_a_large_copy(engine):
    """16,384 tiles or more (here 1,050,000 Gaussian rows of 32 columns, which prune nothing): k <= 7 falls back, k = 8 does not"""
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((1050000, 32), dtype=np.float32)
    q = rng.standard_normal((7, 32), dtype=np.float32)
    p = Pair(engine, rows, 4, max_iter=1)
    try:
        assert p.info["tiles"] >= 16384
        for k in (5, 7):
            _, st = p.check(q, k, "large copy, k = %d" % k)
            assert st["seeds"] > 0 and st["visited"] == st["total"] + st["seeds"], st
        _, st = p.check(q, 8, "large copy, k = 8")
        assert st["visited"] <= p.info["tiles"] < st["total"] + st["seeds"], st
    finally:
        p.free()


# ---- downstream ----

def test_query_rows_and_neighbour_graph(model, engine):
    from scann.models import latent_index
    from scann.models.latent_index import LatentIndex

    rng = np.random.default_rng(6)
    rows = clustered(rng, 700, 128)
    rows[100] = rows[10]
    index = LatentIndex(model, "atom").add_rows(rows)
    try:
        for part in (None, 7):
            if part:
                info = index.partition(part)
                assert info["cells"] == 7 and 0 <= info["pad_share"] < 0.5 and index.partition_args() == (7, 8)
            for first, n in ((0, 700), (64, 65), (699, 1)):
                got = engine.index_query_rows(index._ix, first, n, 5)
                same_dict(got, engine.index_query(index._ix, engine.index_read(index._ix, first, n)[0], 5), "query_rows %d %d" % (first, n))
            pos, d2 = latent_index.neighbour_graph(index, chunk=256)
            hpos, hd2 = latent_index.neighbour_graph_host(rows)
            assert np.array_equal(pos, hpos) and np.array_equal(_bits(d2), _bits(hd2))
        assert index.search_stats()["visited_share"] <= 1.0
        with pytest.raises(ValueError):
            index.partition("many")
        assert index.drop_partition().partition_args() is None
    finally:
        index.free()
    # two storage chunks: the queries of one call come from both
    wide = clustered(rng, 16500, 1024, spread=3.0)
    ix = engine.index_create(1024)
    try:
        engine.index_add(ix, wide)
        engine.index_partition(ix, 4, 1)
        got = engine.index_query_rows(ix, 16380, 8, 3)
        same_dict(got, engine.index_query(ix, wide[16380:16388], 3), "query_rows across chunks")
        assert np.array_equal(got["position"][:, 0], np.arange(16380, 16388))
    finally:
        ix.free()


def test_save_and_load_rebuild_the_partition(model, engine, tmp_path):
    from scann.models.latent_index import LatentIndex

    rng = np.random.default_rng(15)
    rows = clustered(rng, 900, 128)
    index = LatentIndex(model, "atom").add_rows(rows, np.arange(900) // 30, np.arange(900) % 30)
    try:
        index.partition(9, max_iter=3)
        before = engine.index_cells_read(index._ix)
        index.add_rows(rows[:0])  # no row: the partition stays, and the index says so
        assert index.partition_args() == (9, 3) and engine.index_cells_read(index._ix)["cells"] == 9
        index.save(str(tmp_path / "cut.npz"))
        with np.load(str(tmp_path / "cut.npz")) as z:
            assert np.array_equal(z["partition"], [9, 3])
        again = LatentIndex.load(model, str(tmp_path / "cut.npz"))
        try:
            assert again.partition_args() == (9, 3) and len(again) == 900
            cells_ref.same(engine.index_cells_read(again._ix), before, "save / load")
            q = rows[:40] + np.float32(0.01)
            same_dict(engine.index_query(again._ix, q, 5), engine.index_query(index._ix, q, 5), "save / load")
        finally:
            again.free()
        engine.index_partition(index._ix, 4, 1)  # behind the LatentIndex's back: it still reports what the index has
        assert index.partition_args() == (4, 1)
        index.add_rows(rows[:3])
        assert index.partition_args() is None
        index.save(str(tmp_path / "plain.npz"))
        with np.load(str(tmp_path / "plain.npz")) as z:
            assert "partition" not in z.files
    finally:
        index.free()


def test_selected_outputs_and_training_state_are_untouched(hip_lib, model):
    """as tests/test_gpu_hier.py and tests/test_gpu_ranks.py check their calls: a batch's last y and selected outputs stay where they
    were across partition + search, and a training handle's gradients, weights and next (deterministic) step are those of a twin handle
    that never partitioned or searched"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    eng, data = model.engine, model.inputs24
    rng = np.random.default_rng(16)
    rows = clustered(rng, 600, 128)
    names = ["local_attention_1", "after_Lc"]
    before = model.predict(data, outputs=names)
    eng.set_outputs([1], after_lc=True)
    try:
        rb = eng.upload(_hip.pack_inputs(data))
        eng.forward_resident(rb)
        y_first, _ = eng.download(rb)
        sel0 = [eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 1), eng.read_output(rb, _hip.OUT_AFTER_LC)]
        ix = eng.index_create(128)
        eng.index_add_batch(ix, rb, _hip.OUT_AFTER_LC)
        eng.forward_resident(rb)
        eng.download(rb)
        eng.index_partition(ix, 5, 2)
        eng.index_query(ix, rows[:30], 5)
        eng.index_query_rows(ix, 0, 20, 32)
        y_again, _ = eng.download(rb)
        assert np.array_equal(_bits(y_again), _bits(y_first))
        assert np.array_equal(_bits(eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 1)), _bits(sel0[0]))
        assert np.array_equal(_bits(eng.read_output(rb, _hip.OUT_AFTER_LC)), _bits(sel0[1]))
        with pytest.raises(_hip.ScannHipError):
            eng.read_output(rb, _hip.OUT_BF_PROPERTY)  # still not selected
        rb.free()
        ix.free()
    finally:
        eng.set_outputs()
    after = model.predict(data, outputs=names)
    assert all(np.array_equal(_bits(x), _bits(y_)) for x, y_ in zip(before, after))
    # a training handle
    cfg = so.default_config("qm9")
    w = so.init_weights(cfg, 1234, perturb=True)
    small, _ = so.pad_batch(*so.synth_dataset(8, 5, kind="qm9"), g_update=cfg["model"]["g_update"])
    pk = _hip.pack_inputs({k: np.array(v) for k, v in small.items()})
    targets = np.linspace(-1, 1, pk.n_struct).astype(np.float32)
    res = []
    for i in range(2):
        te = HipModel(cfg, w, device=0, deterministic=True).engine
        te.train_begin()
        rb = te.upload(pk)
        te.train_step(rb, targets, 1e-3, dropout=0.1, seed=3)
        te.train_step(rb, targets, 1e-3, dropout=0.1, seed=4)
        if i == 0:
            p = Pair(te, rows, 7)
            try:
                p.check(rows[:140] + np.float32(0.01), 5, "training handle")
                p.check(rows[:140] + np.float32(0.01), 32, "training handle")
            finally:
                p.free()
        grads, weights = te.get_grads(), te.get_weights()
        step = te.train_step(rb, targets, 1e-3, dropout=0.1, seed=5)
        res.append((grads, weights, step, te.get_weights()))
        rb.free()
        te.close()
    (ga, wa, sa, wa2), (gb, wb, sb_, wb2) = res
    for key in ga:
        assert np.array_equal(_bits(ga[key]), _bits(gb[key])), key
        assert np.array_equal(_bits(wa[key]), _bits(wb[key])), key
        assert np.array_equal(_bits(wa2[key]), _bits(wb2[key])), key
    assert sa == sb_


def test_select_against_a_partitioned_reference(engine):
    rng = np.random.default_rng(13)
    pool_rows, ref_rows = clustered(rng, 600, 33), clustered(rng, 900, 33)
    pool = engine.index_create(33)
    p = Pair(engine, ref_rows, 7)
    try:
        engine.index_add(pool, pool_rows)
        same_dict(engine.index_select(pool, p.plain, 20), engine.index_select(pool, p.cut, 20), "select")
        st = engine.index_search_stats(p.cut)
        assert st["groups"] == 5 and st["total"] == 5 * 15
    finally:
        pool.free()
        p.free()


def test_model_calls_are_unchanged_by_a_partition(model):
    inputs = model.inputs24
    w0 = model.engine.get_weights()
    y0, ga0 = model.predict(inputs)
    index = model.build_index(inputs, level="atom")
    cut = model.build_index(inputs, level="atom", cells=7)
    try:
        assert cut.partition_args() == (7, 8) and index.partition_args() is None and len(cut) == len(index)
        _, emb = index.embed(perplexity=5, iterations=(5, 5))
        _, hier = index.hierarchy(min_samples=3)
        n_exc = np.arange(24, dtype=np.int64)
        plain = [model.nearest(inputs, index, k=5), model.nearest(inputs, index, k=3, exclude_ids=n_exc), model.place(inputs, emb, index),
                 model.attach(inputs, hier, index, 5)]
        index.partition(7)
        again = [model.nearest(inputs, index, k=5), model.nearest(inputs, index, k=3, exclude_ids=n_exc), model.place(inputs, emb, index),
                 model.attach(inputs, hier, index, 5)]
        assert index.search_stats()["groups"] > 0
        for a, b, name in zip(plain, again, ("nearest", "nearest, leave-one-out", "place", "attach")):
            same_dict(a, b, name)
        same_dict(plain[0], model.nearest(inputs, cut, k=5), "build_index(cells=7)")
        assert np.array_equal(_bits(plain[0]["predict_property"]), _bits(y0))
        with pytest.raises(ValueError):
            model.build_index(inputs, level="atom", cells=2000)
    finally:
        index.free()
        cut.free()
    y1, ga1 = model.predict(inputs)
    assert np.array_equal(_bits(y0), _bits(y1)) and np.array_equal(_bits(ga0), _bits(ga1))
    w1 = model.engine.get_weights()
    for key in w0:
        assert np.array_equal(_bits(w0[key]), _bits(w1[key])), key


def test_other_analyses_never_read_the_copy(engine):
    rng = np.random.default_rng(14)
    rows = clustered(rng, 400, 33)
    ids = (np.arange(400) // 20).astype(np.int64)
    p = Pair(engine, rows, 7, ids, (np.arange(400) % 20).astype(np.int32))
    try:
        labels = (np.arange(400) % 3).astype(np.int32)
        probe = rng.integers(0, 400, (400, 4)).astype(np.int32)
        calls = {"match": lambda ix: engine.index_match(ix, rows[:30], np.array([0, 12, 30], np.int32), 3),
                 "kmeans": lambda ix: engine.index_kmeans(ix, np.array([0, 5, 9], np.int32), 5),
                 "density": lambda ix: {"sum": engine.index_density(ix, rows[:16], 0.05)},
                 "mst": lambda ix: engine.index_mst(ix),
                 "silhouette": lambda ix: engine.index_silhouette(ix, labels, 3),
                 "ranks": lambda ix: engine.index_ranks(ix, probe, dist2=True)}
        for name, call in calls.items():
            same_dict(call(p.plain), call(p.cut), name)
        assert engine.index_cells_read(p.cut)["cells"] == 7
    finally:
        p.free()


def test_errors_before_any_launch(hip_lib, engine):
    from scann import _hip
    from scann.models.scann_model import HipModel

    ix = engine.index_create(8)
    engine.index_add(ix, np.zeros((10, 8), np.float32))
    cfg = so.default_config("qm9")
    other = HipModel(cfg, so.init_weights(cfg, 1, perturb=True), device=0, infer=True)
    try:
        info = np.zeros(4, np.int64)
        for cells, it in ((-1, 1), (1025, 1), (4, -1)):
            assert hip_lib.scann_index_partition(engine._h, ix._h, cells, it, info.ctypes.data) == -1
            assert engine.index_cells_read(ix)["cells"] == 0
        assert hip_lib.scann_index_partition(other.engine._h, ix._h, 4, 1, info.ctypes.data) == -1  # an index of another handle
        out = engine._knn_out(1, 1)
        for first, n, k in ((-1, 1, 1), (5, 6, 1), (0, 0, 1), (0, 1, 0), (0, 1, 33)):
            assert hip_lib.scann_index_query_rows(engine._h, ix._h, first, n, k, out["dist2"].ctypes.data, None, None, None) == -1
        with pytest.raises(ValueError):
            engine.index_partition(ix, -1)
        with pytest.raises(_hip.ScannHipError):
            other.engine.index_partition(ix, 4)
    finally:
        other.engine.close()
        ix.free()

"""GPU tests of the radius search over a latent-space index (scann_index_within, scann_index_within_rows, scann_index_within_batch through
Engine.index_within*, LatentIndex.within / duplicates, HipModel.within / duplicates, predict_model.py --within / --duplicates).

Every comparison is of bytes: the device equals the host twin (scann_within_host) and the NumPy restatement of the definition
(tests/within_ref.py) in counts, total and the four entry arrays, and the device with a partition equals the device without one.
Radii come from the case's own distance matrix: 0 with planted exact copies, a value that IS a distance of the case (the inclusive
boundary), the quantile that gives about 10 hits per query, and +inf at N <= 1,000.
1. Sizes round the tile (63, 64, 65), several groups of queries, cells > N, two storage chunks, several adds; integer grids where many
   pairs tie at exactly radius2; non-finite rows and queries; query ids.  2. The self-join: ``upper`` 0 and 1, first > 0, across chunks.
3. The size-then-fill protocol on the C call; an empty index.  4. The plan skips on blobs.  5. Model level on the synthetic qm9 and mp2018
   sets; duplicates; generic widths and a training handle; non-interference; memory; errors; the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import scann_oracle as so  # noqa: E402
import within_ref  # noqa: E402
from analysis_checks import _bits, amask_of, padded, setup, steady_memory  # noqa: E402
from test_cells_host import blobs  # noqa: E402
from test_gpu_cells import clustered  # noqa: E402
from test_gpu_knn import reps_of  # noqa: E402
from test_within_host import radii_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hip_lib):
    cfg, w, inputs, m = setup(n=24)
    m.inputs24 = inputs
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def engine(model):
    return model.engine


def same_result(got, want, label):
    for key in ("count", "first", "position", "id", "atom", "dist2"):
        if key in want:
            a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (label, key)
    assert got["total"] == want["total"], label


class Case:
    """rows in an index, searched without a partition and with each of ``cells``"""

    def __init__(self, eng, rows, ids=None, atoms=None, adds=1):
        self.eng, self.rows = eng, np.ascontiguousarray(rows, np.float32)
        n = len(rows)
        self.ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.atoms = np.full(n, -1, np.int32) if atoms is None else np.asarray(atoms, np.int32)
        self.ix = eng.index_create(rows.shape[1])
        cuts = np.linspace(0, n, adds + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng.index_add(self.ix, self.rows[a:b], self.ids[a:b], self.atoms[a:b])

    def free(self):
        self.ix.free()

    def layouts(self, cells):
        """the index without a partition, then with each number of cells; the partition is dropped at the end"""
        yield "no partition"
        for c in cells:
            self.eng.index_partition(self.ix, c, 4)
            yield "%d cells" % c
        self.eng.index_partition(self.ix, 0, 0)

    def check(self, q, radii, cells, label, query_ids=None):
        """index_within on every layout == the twin == the restated definition, in every byte"""
        from scann import _hip

        q = np.ascontiguousarray(q, np.float32)
        with np.errstate(all="ignore"):
            d = _hip.knn_dist2_matrix(q, self.rows)
        wants = []
        for r2 in radii:
            want = within_ref.within(d, r2, ids=self.ids, query_ids=query_ids)
            twin = _hip.within_host(self.rows, q, r2, row_ids=self.ids, query_ids=query_ids, max_pairs=1 << 26)
            within_ref.same(twin, want, "%s: the twin, radius2 %r" % (label, r2))
            want["id"], want["atom"] = self.ids[want["position"]], self.atoms[want["position"]]
            wants.append(want)
        for layout in self.layouts(cells):
            for r2, want in zip(radii, wants):
                got = self.eng.index_within(self.ix, q, r2, query_ids=query_ids, max_pairs=1 << 26)
                st = self.eng.index_search_stats(self.ix)
                print("%s, %s: N %d, dim %d, Q %d, radius2 %r: %d hits, visited %d of %d pairs" % (
                    label, layout, len(self.rows), q.shape[1], len(q), r2, got["total"], st["visited"], st["total"]))
                same_result(got, want, "%s, %s, radius2 %r" % (label, layout, r2))
                assert st["seeds"] == 0 and st["visited"] <= st["total"] + st["groups"] * 1025 and st["groups"] == -(-len(q) // 128)
                counted = self.eng.index_within(self.ix, q, r2, query_ids=query_ids, count_only=True)
                assert "dist2" not in counted and np.array_equal(counted["count"], want["count"])
        return wants


# N, dim, cells, Q: N in {1, 63, 64, 65, 130, 1,000, 5,000}, dim in {1, 2, 33, 128, 130}, cells in {1, 7, 64} and cells > N,
# Q in {1, 7, 128, 129, 300}; and one index of 1,024 columns and 17,000 rows that spans two storage chunks
EXACT_CASES = [(1, 1, (1,), 1), (1, 128, (7,), 7), (63, 2, (1, 64), 129), (64, 128, (1, 7), 7), (64, 2, (7,), 128), (65, 130, (7, 200), 129),
               (65, 1, (64,), 300), (130, 33, (7, 200), 128), (1000, 128, (1, 64), 300), (1000, 1, (7,), 129), (1000, 130, (7,), 128),
               (5000, 128, (64,), 129), (5000, 33, (7,), 300), (5000, 2, (64,), 1), (17000, 1024, (7,), 7)]


@pytest.mark.parametrize("N,dim,cells,Q", EXACT_CASES, ids=["N%d_d%d_c%s_Q%d" % (n, d, "-".join(map(str, c)), q) for n, d, c, q in EXACT_CASES])
def test_within_is_exact(engine, N, dim, cells, Q):
    from scann import _hip

    rng = np.random.default_rng(N * 7 + dim * 3 + Q)
    rows = clustered(rng, N, dim)
    if N >= 63:
        rows[N // 2] = rows[3]  # an exact copy within the index
    ids = rng.integers(0, 1 << 40, N).astype(np.int64)
    atoms = rng.integers(-1, 30, N).astype(np.int32)
    near = rows[rng.integers(0, N, Q - Q // 2)] + np.float32(0.05) * rng.standard_normal((Q - Q // 2, dim)).astype(np.float32)
    near[::3] = rows[rng.integers(0, N, len(near[::3]))]  # exact copies of rows among the queries: hits at radius 0
    q = np.concatenate([near, clustered(rng, Q // 2, dim)]).astype(np.float32)
    c = Case(engine, rows, ids, atoms)
    try:
        radii = radii_of(_hip.knn_dist2_matrix(q, rows))
        if N > 1000:
            radii = radii[:-1]  # +inf at N <= 1,000
        wants = c.check(q, radii, cells, "clustered")
        assert wants[0]["total"] >= len(near[::3]) and (wants[1]["dist2"] == np.float32(radii[1])).any()  # copies at 0; the boundary is met
    finally:
        c.free()


def test_an_index_built_by_several_adds_and_query_ids(engine):
    rng = np.random.default_rng(21)
    rows = clustered(rng, 700, 33)
    ids = (np.arange(700) // 25).astype(np.int64)
    c = Case(engine, rows, ids, (np.arange(700) % 25).astype(np.int32), adds=5)
    try:
        q = rows[rng.integers(0, 700, 140)] + np.float32(0.01)
        from scann import _hip

        radii = radii_of(_hip.knn_dist2_matrix(q, rows))
        c.check(q, radii, (7,), "several adds")
        c.check(q, radii[1:3], (7,), "query ids", query_ids=rng.integers(0, 28, 140).astype(np.int64))
        one = Case(engine, rows, np.zeros(700, np.int64))
        try:
            assert one.check(q, [np.inf], (3,), "one id for all", query_ids=np.zeros(140, np.int64))[0]["total"] == 0
        finally:
            one.free()
    finally:
        c.free()


def test_first_k_hits_are_the_nearest_rows_where_they_qualify(engine):
    rng = np.random.default_rng(25)
    rows = rng.integers(0, 5, (900, 3)).astype(np.float32)  # ties within and across the radius
    q = rng.integers(0, 5, (140, 3)).astype(np.float32)
    ids, qid = rng.integers(0, 6, 900).astype(np.int64), rng.integers(0, 6, 140).astype(np.int64)
    c = Case(engine, rows, ids)
    try:
        for layout in c.layouts((7,)):
            knn = engine.index_query(c.ix, q, 32, query_ids=qid)
            for r2 in (0.0, 2.0, 6.0):
                got = engine.index_within(c.ix, q, r2, query_ids=qid)
                for i in range(140):
                    m = min(32, int(got["count"][i]))
                    s = slice(got["first"][i], got["first"][i] + m)
                    assert np.array_equal(got["position"][s], knn["position"][i, :m]) and np.array_equal(_bits(got["dist2"][s]), _bits(knn["dist2"][i, :m]))
                    assert np.array_equal(got["id"][s], knn["id"][i, :m]) and (m == 32 or not knn["dist2"][i, m] <= r2), (layout, r2, i)
    finally:
        c.free()


def test_ties_at_exactly_the_radius_and_non_finite_values(engine):
    rng = np.random.default_rng(22)
    grid = rng.integers(0, 4, (1500, 2)).astype(np.float32)
    c = Case(engine, grid)
    try:
        wants = c.check(rng.integers(0, 4, (129, 2)).astype(np.float32), [0.0, 1.0, 2.0, 5.0], (7, 64), "grid")
        assert all((w["dist2"] == r2).sum() > 1000 for w, r2 in zip(wants, (0.0, 1.0, 2.0, 5.0)))
    finally:
        c.free()
    cube = np.zeros((900, 130), np.float32)
    cube[:, 60:70] = rng.integers(0, 2, (900, 10))  # the ties lie in the third of five slabs
    c = Case(engine, cube)
    try:
        c.check(cube[:140], [0.0, 3.0], (9,), "cube")
    finally:
        c.free()
    rows = clustered(rng, 400, 5)
    rows[0, 0], rows[200, 4], rows[399, 0], rows[77] = np.nan, np.inf, -np.inf, 3e19
    q = rows[rng.integers(0, 400, 70)].copy()
    q[4, 0], q[9, 1] = np.nan, np.inf
    c = Case(engine, rows)
    try:
        wants = c.check(q, [0.0, 2.0, 3e38, np.inf], (1, 4), "non-finite")
        assert wants[3]["count"][4] == 0 and np.isposinf(wants[3]["dist2"]).any() and not np.isposinf(wants[2]["dist2"]).any()
    finally:
        c.free()


# ---- 2. the self-join ----

def check_rows(c, first, n, r2, cells, label):
    from scann import _hip

    with np.errstate(all="ignore"):
        d = _hip.knn_dist2_matrix(c.rows[first:first + n], c.rows)
    qpos = np.arange(first, first + n, dtype=np.int32)
    wants = {}
    for upper in (0, 1):
        want = within_ref.within(d, r2, query_pos=qpos, upper=upper)
        within_ref.same(_hip.within_host(c.rows, c.rows[first:first + n], r2, query_pos=qpos, upper=upper, max_pairs=1 << 26), want, label + ": the twin")
        want["id"], want["atom"] = c.ids[want["position"]], c.atoms[want["position"]]
        wants[upper] = want
    for layout in c.layouts(cells):
        for upper in (0, 1):
            got = c.eng.index_within_rows(c.ix, first, n, r2, upper=upper, max_pairs=1 << 26)
            st = c.eng.index_search_stats(c.ix)
            print("%s, %s, upper %d: rows %d .. %d of %d, radius2 %r: %d hits, visited %d of %d pairs" % (
                label, layout, upper, first, first + n, len(c.rows), r2, got["total"], st["visited"], st["total"]))
            same_result(got, wants[upper], "%s, %s, upper %d" % (label, layout, upper))
            if layout == "no partition":  # below the diagonal nothing is visited
                assert st["visited"] == st["total"] if not upper else st["visited"] <= st["total"]
                if upper and first + n == len(c.rows) and n >= 256:
                    assert st["visited"] < st["total"]
    return wants


def test_rows_of_the_index_as_queries(engine):
    rng = np.random.default_rng(23)
    rows = rng.integers(0, 6, (1000, 3)).astype(np.float32)
    c = Case(engine, rows, adds=3)
    try:
        for first, n in ((0, 1000), (64, 65), (999, 1), (300, 700)):
            w = check_rows(c, first, n, 1.0, (7,), "grid self-join")
        whole = check_rows(c, 0, 1000, 2.0, (64,), "grid self-join")
        assert whole[0]["total"] == 2 * whole[1]["total"] > 1000  # every unordered pair once
        i = np.repeat(np.arange(1000), whole[1]["count"])
        assert np.all(i < whole[1]["position"])
    finally:
        c.free()
    # two storage chunks: the queries of one call come from both, and the hits too
    wide = clustered(rng, 16500, 1024, spread=3.0)
    wide[16390], wide[5] = wide[16382], wide[16385]
    c = Case(engine, wide)
    try:
        w = check_rows(c, 16380, 8, 0.0, (4,), "across chunks")
        assert w[0]["position"].tolist() == [16390, 5] and w[1]["position"].tolist() == [16390]  # (rows 16390 and 5 are no queries)
    finally:
        c.free()


# ---- 3. the protocol, an empty index ----

def test_size_then_fill_protocol_on_the_device(hip_lib, engine):
    from scann import _hip

    rng = np.random.default_rng(24)
    rows = rng.integers(0, 4, (300, 2)).astype(np.float32)
    q = rng.integers(0, 4, (50, 2)).astype(np.float32)
    want = within_ref.within(_hip.knn_dist2_matrix(q, rows), 1.0)
    total = want["total"]
    c = Case(engine, rows)

    def call(cap, arrays=True):
        counts, tot = np.full(50, -1, np.int64), np.full(1, -1, np.int64)
        d, p, i, a = np.full(total + 1, -7, np.float32), np.full(total + 1, -7, np.int32), np.full(total + 1, -7, np.int64), np.full(total + 1, -7, np.int32)
        r = hip_lib.scann_index_within(engine._h, c.ix._h, q.ctypes.data, 50, None, 1.0, cap, counts.ctypes.data, tot.ctypes.data,
                                       *([x.ctypes.data for x in (d, p, i, a)] if arrays else [None] * 4))
        return r, counts, int(tot[0]), d, p, i, a

    try:
        for layout in c.layouts((5,)):
            r, counts, tot, d, p, i, a = call(total)  # cap = total fills
            assert r == 0 and tot == total and np.array_equal(counts, want["count"]), layout
            assert np.array_equal(p[:total], want["position"]) and np.array_equal(_bits(d[:total]), _bits(want["dist2"])) and p[total] == -7
            assert np.array_equal(i[:total], want["position"]) and np.all(a[:total] == -1) and i[total] == -7 and a[total] == -7
            r, counts, tot, d, p, i, a = call(total - 1)  # one short: counts and total exact, nothing else touched, still SCANN_OK
            assert r == 0 and tot == total and np.array_equal(counts, want["count"]), layout
            assert np.all(d == -7) and np.all(p == -7) and np.all(i == -7) and np.all(a == -7)
            r, counts, tot, *_ = call(0, arrays=False)  # count only
            assert r == 0 and tot == total and np.array_equal(counts, want["count"])
        with pytest.raises(ValueError, match="max_pairs is %d" % (total - 1)):
            engine.index_within(c.ix, q, 1.0, max_pairs=total - 1)
        assert engine.index_within(c.ix, q, 1.0, max_pairs=total)["total"] == total
        big = np.zeros((30, 2), np.float32)  # more hits than the wrapper's first cap: the second call is sized by the first
        zero = Case(engine, np.zeros((400, 2), np.float32))
        try:
            got = engine.index_within(zero.ix, big, 0.0)
            assert got["total"] == 12000 and np.array_equal(got["position"], np.tile(np.arange(400, dtype=np.int32), 30))
        finally:
            zero.free()
    finally:
        c.free()


def test_an_empty_index_gives_zeros(engine):
    ix = engine.index_create(8)
    try:
        got = engine.index_within(ix, np.zeros((5, 8), np.float32), np.inf)
        assert got["total"] == 0 and not got["count"].any() and got["first"].tolist() == [0] * 6 and got["position"].shape == (0,)
        assert engine.index_search_stats(ix) == {"total": 0, "seeds": 0, "visited": 0, "groups": 0}
    finally:
        ix.free()


# ---- 4. the plan skips ----

def test_the_plan_skips_on_blobs(engine):
    from scann import _hip

    rows, q = blobs()
    c = Case(engine, rows)
    try:
        engine.index_partition(c.ix, 8, 4)
        got = engine.index_within(c.ix, q, 40.0)
        st = engine.index_search_stats(c.ix)
        print("blobs, 256 queries: %d hits, visited %d of %d pairs" % (got["total"], st["visited"], st["total"]))
        within_ref.same(got, within_ref.within(_hip.knn_dist2_matrix(q, rows), 40.0), "blobs")
        assert got["total"] == 6338 and st["groups"] == 2 and st["total"] == 128 and st["seeds"] == 0 and 4 * st["visited"] <= st["total"], st
        up = engine.index_within_rows(c.ix, 0, 4096, 40.0, upper=1)
        st = engine.index_search_stats(c.ix)
        print("blobs, self-join: %d pairs, visited %d of %d pairs" % (up["total"], st["visited"], st["total"]))
        within_ref.same(up, _hip.within_host(rows, rows, 40.0, query_pos=np.arange(4096, dtype=np.int32), upper=1), "blobs self-join")
        assert st["groups"] == 32 and st["total"] == 2048 and 2 * st["visited"] <= st["total"], st
    finally:
        c.free()


# ---- 5. the model level ----

E2E = {"qm9": (48, 16), "mp2018": (20, 8)}


@pytest.mark.parametrize("level", ["structure", "atom"])
@pytest.mark.parametrize("kind", ["qm9", "mp2018"])
def test_model_within_is_the_search_on_the_models_rows(hip_lib, kind, level):
    from scann import _hip

    n_i, n_q = E2E[kind]
    cfg, w, data, model = setup(kind=kind, n=n_i, seed=0)
    queries = padded(kind, n_q, 1, cfg)
    try:
        ix = model.build_index(data, level=level, batch_size=16)
        y, ga = model.predict(queries)
        qrows = reps_of(model, queries, level)
        qm = amask_of(queries)
        d = _hip.knn_dist2_matrix(qrows, ix.rows()[0])
        for layout in ("no partition", "3 cells"):
            if layout != "no partition":
                ix.partition(3)
            for r2 in radii_of(d):
                radius = float(np.sqrt(np.float64(r2)))
                if latent_radius2(radius) != np.float32(r2):
                    continue  # (a radius whose fp32 square is another threshold: the direct call below would differ by design)
                direct = ix.within(qrows, radius, max_pairs=1 << 26)
                within_ref.same(direct, within_ref.within(d, r2), "%s %s %s radius2 %r" % (kind, level, layout, r2))
                got = model.within(queries, ix, radius, batch_size=5, max_pairs=1 << 26)
                assert np.array_equal(_bits(got["predict_property"]), _bits(y))
                cnt = got["count"] if level == "structure" else got["count"][qm]
                assert np.array_equal(cnt, direct["count"]) and np.array_equal(got["first"], direct["first"]) and got["count"].dtype == np.int64
                if level == "atom":
                    assert got["count"].shape == qm.shape and not got["count"][~qm].any()
                for a, b in (("position", "position"), ("neighbor_id", "id"), ("neighbor_atom", "atom"), ("dist2", "dist2"), ("distance", "distance")):
                    assert got[a].dtype == direct[b].dtype and got[a].tobytes() == direct[b].tobytes(), (a, layout, r2)
                only = model.within(queries, ix, radius, count_only=True)
                assert sorted(only) == ["count", "first", "predict_property"] and np.array_equal(only["count"], got["count"])
        # y and the scores of the batch call are the plain forward's; exclude_ids leave the structure's own rows out
        rb = model.engine.upload(_hip.pack_inputs(queries))
        r = model.engine.index_within_batch(ix._ix, rb, _hip.KNN_LEVELS[level], 0.0)
        rb.free()
        assert np.array_equal(_bits(r["y"]), _bits(y[:, 0])) and np.array_equal(_bits(r["ga"]), _bits(ga[qm][:, 0]))
        me = model.within(data, ix, 0.0)
        loo = model.within(data, ix, 0.0, exclude_ids=np.arange(n_i))
        dm = amask_of(data)
        own = np.arange(n_i) if level == "structure" else np.repeat(np.arange(n_i), dm.sum(1))  # the structure of every query row
        cnt = me["count"] if level == "structure" else me["count"][dm]
        mine = me["neighbor_id"] == np.repeat(own, cnt)
        assert np.all(cnt >= 1) and np.all(np.add.reduceat(mine, me["first"][:-1]) >= 1)  # every row finds itself at distance 0
        cnt1 = loo["count"] if level == "structure" else loo["count"][dm]
        assert loo["first"][-1] == me["first"][-1] - mine.sum() and not np.any(loo["neighbor_id"] == np.repeat(own, cnt1))
        ix.free()
    finally:
        model.engine.close()


def latent_radius2(radius):
    from scann.models import latent_index

    return np.float32(latent_index.radius2_of(radius))


def test_duplicates_pair_every_row_with_its_copy(hip_lib, model):
    inputs = model.inputs24
    twice = {k: np.concatenate([v, v]) for k, v in inputs.items()}
    for level in ("structure", "atom"):
        ix = model.build_index(twice, level=level, batch_size=16)
        try:
            n = len(ix) // 2
            for layout in ("no partition", "5 cells"):
                if layout != "no partition":
                    ix.partition(5)
                dev = ix.duplicates(0.0, chunk=100)
                host = ix.duplicates(0.0, route="host")
                assert sorted(dev) == sorted(host) == ["distance", "group", "keep", "n_groups", "pairs", "sizes"]
                for key in dev:
                    a, b = np.asarray(dev[key]), np.asarray(host[key])
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (level, layout, key)
                pairs = set(map(tuple, dev["pairs"].tolist()))
                assert all((i, i + n) in pairs for i in range(n)) and not dev["distance"].any()
                assert np.array_equal(dev["group"][n:], dev["group"][:n]) and not dev["keep"][n:].any() and dev["n_groups"] <= n
            again = model.duplicates(twice, 0.0, level=level, batch_size=16)
            assert again["pairs"].tobytes() == dev["pairs"].tobytes() and again["group"].tobytes() == dev["group"].tobytes()
            loose = ix.duplicates(0.05, chunk=37)
            assert loose["pairs"].tobytes() == ix.duplicates(0.05, route="host")["pairs"].tobytes() and len(loose["pairs"]) >= len(dev["pairs"])
            with pytest.raises(ValueError, match="max_pairs"):
                ix.duplicates(0.0, max_pairs=n - 1)
        finally:
            ix.free()


def test_generic_width_and_training_handle(hip_lib):
    """a model of generic widths; and a training handle whose gradients, weights and next (deterministic) step are those of a twin handle
    that never searched"""
    from scann import _hip
    from scann.models.scann_model import HipModel

    cfg, w, data, model = setup(n=9, seed=41, local_dim=64, num_head=4, global_dim=96, dense_out=30)
    try:
        for level in ("structure", "atom"):
            ix = model.build_index(data, level=level)
            rows = ix.rows()[0]
            d = _hip.knn_dist2_matrix(rows, rows)
            r2 = float(np.sort(d[d > 0])[len(rows)])
            direct = model.engine.index_within(ix._ix, rows, r2)
            within_ref.same(direct, within_ref.within(d, r2), "generic " + level)
            rb = model.engine.upload(_hip.pack_inputs(data))
            got = model.engine.index_within_batch(ix._ix, rb, _hip.KNN_LEVELS[level], r2)
            rb.free()
            same_result(got, direct, "generic, behind the forward, " + level)
            ix.free()
    finally:
        model.engine.close()
    cfg = so.default_config("qm9")
    w = so.init_weights(cfg, 1234, perturb=True)
    small, _ = so.pad_batch(*so.synth_dataset(8, 5, kind="qm9"), g_update=cfg["model"]["g_update"])
    pk = _hip.pack_inputs({k: np.array(v) for k, v in small.items()})
    targets = np.linspace(-1, 1, pk.n_struct).astype(np.float32)
    rows = clustered(np.random.default_rng(16), 600, 128)
    res = []
    for i in range(2):
        te = HipModel(cfg, w, device=0, deterministic=True).engine
        te.train_begin()
        rb = te.upload(pk)
        te.train_step(rb, targets, 1e-3, dropout=0.1, seed=3)
        te.train_step(rb, targets, 1e-3, dropout=0.1, seed=4)
        if i == 0:
            c = Case(te, rows)
            try:
                c.check(rows[:140] + np.float32(0.01), [0.0, 30.0], (7,), "training handle")
                got = te.index_within_batch(c.ix, rb, _hip.OUT_AFTER_LC, 1e30)
                assert got["total"] == pk.n_atom * 600
            finally:
                c.free()
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


def test_selected_outputs_and_weights_are_untouched(model):
    from scann import _hip

    eng, data = model.engine, model.inputs24
    names = ["local_attention_1", "after_Lc"]
    before = model.predict(data, outputs=names)
    w0 = eng.get_weights()
    eng.set_outputs([1], after_lc=True)
    try:
        rb = eng.upload(_hip.pack_inputs(data))
        eng.forward_resident(rb)
        y_first, _ = eng.download(rb)
        sel0 = [eng.read_output(rb, _hip.OUT_LOCAL_ATTENTION, 1), eng.read_output(rb, _hip.OUT_AFTER_LC)]
        ix = eng.index_create(128)
        eng.index_add_batch(ix, rb, _hip.OUT_AFTER_LC)
        n0 = len(ix)
        for part in (0, 5):
            eng.index_partition(ix, part, 2)
            eng.index_within(ix, sel0[1][:30], 0.5)
            eng.index_within_rows(ix, 0, 20, 0.5, upper=1)
            eng.index_within_batch(ix, rb, _hip.OUT_AFTER_LC, 0.5)
        assert len(ix) == n0 and eng.index_partition_args(ix) == (5, 2)  # the index itself is as it was
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
    w1 = eng.get_weights()
    for key in w0:
        assert np.array_equal(_bits(w0[key]), _bits(w1[key])), key


def test_repeated_calls_do_not_eat_device_memory(hip_lib):
    from scann import _hip

    cfg, w, data, model = setup(n=40, seed=2)
    eng = model.engine
    try:
        rb = eng.upload(_hip.pack_inputs(data))
        ix = eng.index_create(128)
        eng.index_add_batch(ix, rb, _hip.OUT_AFTER_LC)
        eng.index_partition(ix, 4, 2)
        first = eng.index_within_batch(ix, rb, _hip.OUT_AFTER_LC, 0.3)
        eng.index_within_rows(ix, 0, len(ix), 0.3, upper=1)

        def call(rep):
            r = eng.index_within_batch(ix, rb, _hip.OUT_AFTER_LC, 0.3) if rep % 2 else eng.index_within_rows(ix, 0, len(ix), 0.3, upper=1)
            if rep % 2:
                assert r["position"].tobytes() == first["position"].tobytes()

        steady_memory(eng, call, 30, 32 << 20)
        rb.free()
        ix.free()
    finally:
        eng.close()


def test_errors_before_any_launch(hip_lib, engine, model):
    from scann import _hip
    from scann.models.scann_model import HipModel

    ix = engine.index_create(8)
    engine.index_add(ix, np.zeros((10, 8), np.float32))
    cfg = so.default_config("qm9")
    other = HipModel(cfg, so.init_weights(cfg, 1, perturb=True), device=0, infer=True)
    rb = engine.upload(_hip.pack_inputs(model.inputs24))
    try:
        q = np.zeros((3, 8), np.float32)
        counts, tot, d = np.zeros(10, np.int64), np.zeros(1, np.int64), np.zeros(4, np.float32)
        cp, tp, dp = counts.ctypes.data, tot.ctypes.data, d.ctypes.data

        def within(h=engine._h, ixh=ix._h, qp=q.ctypes.data, nq=3, r2=1.0, cap=0, c=cp, t=tp, dd=None):
            return hip_lib.scann_index_within(h, ixh, qp, nq, None, r2, cap, c, t, dd, None, None, None)

        def rows(first=0, n=1, upper=0, r2=1.0, cap=0, c=cp, t=tp, dd=None):
            return hip_lib.scann_index_within_rows(engine._h, ix._h, first, n, upper, r2, cap, c, t, dd, None, None, None)

        assert within() == 0 and rows() == 0
        bad = [within(h=None), within(ixh=None), within(h=other.engine._h), within(qp=None), within(nq=0), within(r2=float("nan")), within(r2=-1.0),
               within(cap=-1), within(cap=(1 << 30) + 1), within(dd=dp), within(c=None), within(t=None),
               rows(first=-1), rows(first=5, n=6), rows(n=0), rows(upper=2), rows(upper=-1), rows(r2=-0.5), rows(cap=-1), rows(dd=dp), rows(c=None)]
        assert bad == [-1] * len(bad), bad
        for level, r2, cap, c in ((7, 1.0, 0, cp), (_hip.OUT_BF_PROPERTY, 1.0, 0, cp), (_hip.OUT_AFTER_LC, -1.0, 0, cp), (_hip.OUT_AFTER_LC, 1.0, -1, cp)):
            # a bad level; a width that is not the index's (8 columns); a bad radius2; a bad cap
            assert hip_lib.scann_index_within_batch(engine._h, ix._h, rb._h, level, None, r2, cap, None, None, c, tp, None, None, None, None) == -1
        assert hip_lib.scann_index_within_batch(engine._h, ix._h, None, _hip.OUT_AFTER_LC, None, 1.0, 0, None, None, cp, tp, None, None, None, None) == -1
        for call in (lambda: engine.index_within(ix, q, -1.0), lambda: engine.index_within(ix, q[:, :5], 1.0), lambda: engine.index_within(ix, q, 1.0, max_pairs=-1),
                     lambda: engine.index_within(ix, q, 1.0, query_ids=np.zeros(2)), lambda: engine.index_within_rows(ix, 0, 5, 1.0, upper=3),
                     lambda: engine.index_within_batch(ix, rb, _hip.OUT_AFTER_LC, 1.0, query_ids=np.zeros(3))):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(_hip.ScannHipError):
            other.engine.index_within(ix, q, 1.0)
        index = model.build_index(model.inputs24, level="structure")
        try:
            for call in (lambda: model.within(model.inputs24, index, -1.0), lambda: model.within(model.inputs24, index, np.nan),
                         lambda: model.within(model.inputs24, "index", 1.0), lambda: model.within(model.inputs24, index, 1.0, exclude_ids=np.arange(3)),
                         lambda: model.within(model.inputs24, index, 1.0, batch_size=0), lambda: model.within(model.inputs24, index, 1.0, max_pairs=2.5),
                         lambda: other.within(model.inputs24, index, 1.0), lambda: index.within(np.zeros((2, 3), np.float32), 1.0),
                         lambda: index.duplicates(1.0, route="fast"), lambda: index.duplicates(1.0, chunk=0),
                         lambda: model.duplicates(model.inputs24, 1.0, level="bond"), lambda: model.duplicates(model.inputs24, "x")):
                with pytest.raises(ValueError):
                    call()
        finally:
            index.free()
    finally:
        rb.free()
        ix.free()
        other.engine.close()


def test_cli_reports_duplicates_and_leakage(hip_lib, tmp_path):
    """predict_model.py --duplicates RADIUS prints the groups and the redundant rows and writes the groups; --within RADIUS --within-index
    FILE prints how many of the dataset's structures have an indexed row within RADIUS and pickles the lists; the other files' bytes
    are those of a run without the flags"""
    import yaml

    from scann.models import SCANN
    from scann.models.scann_model import save_container

    n = 20
    de, dn = so.synth_dataset(n, 5)
    de, dn = list(de) + list(de[:5]), list(dn) + list(dn[:5])  # five structures entered twice
    full = np.empty(len(de), dtype=object)
    for i in range(len(de)):
        full[i] = {"Atomic": de[i][0], "Properties": {"homo": float(i)}}
    nei = np.empty(len(dn), dtype=object)
    for i in range(len(dn)):
        nei[i] = dn[i]
    np.save(tmp_path / "data_energy.npy", full, allow_pickle=True)
    np.save(tmp_path / "data_nei.npy", nei, allow_pickle=True)
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
    scann = SCANN(yaml.safe_load(open(out / "config.yaml")), str(out / "models" / "model_homo.h5"), mode="infer")
    scann.prepare_dataset(split=False)
    data = scann.dataIter
    pool = scann.build_index(data, level="structure", ids=data.indexes)
    want = pool.duplicates(0.0)
    pool.save(str(tmp_path / "train.npz"))
    r = subprocess.run(cli + ["--duplicates", "0", "--duplicates-out", str(tmp_path / "groups.pickle"), "--within", "0", "--within-index",
                              str(tmp_path / "train.npz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f, b in plain.items():
        assert open(out / f, "rb").read() == b, f
    assert want["n_groups"] <= 20 and "%d groups, %d redundant rows" % (want["n_groups"], 25 - want["n_groups"]) in r.stdout, r.stdout[-2000:]
    got = pickle.load(open(tmp_path / "groups.pickle", "rb"))
    for key in ("pairs", "group", "keep"):
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
    assert np.array_equal(got["id"], np.asarray(data.indexes))
    assert "25 of 25 structures have an indexed row within" in r.stdout, r.stdout[-2000:]
    leak = pickle.load(open(out / "within_homo.pickle", "rb"))
    direct = scann.within(data, pool, 0.0)
    assert len(leak) == 25 and all(np.array_equal(leak[i]["neighbor_id"], direct["neighbor_id"][direct["first"][i]:direct["first"][i + 1]]) for i in range(25))
    pool.free()
    r = subprocess.run(cli + ["--within", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--within-index" in (r.stdout + r.stderr)
    r = subprocess.run(cli + ["--duplicates", "-1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--duplicates" in (r.stdout + r.stderr)

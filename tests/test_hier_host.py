"""Host tests of the hierarchical clustering of a latent index (scann_index_mst's twin scann_mst_host, LatentIndex.hierarchy,
LatentHierarchy): the twin against the restatement of the definition (tests/hier_ref.py: Kruskal over all pairs) edge for edge and bit
for bit -- Gaussian rows, lattices full of ties, coincident rows, a constant core distance, non-finite rows, overflowing distances --; the
Boruvka restatement against Kruskal; independence of the thread count; heights against SciPy; the crescents with outliers against the
planted labels and scikit-learn's HDBSCAN; blobs of unequal density; cuts; the round trip; the host route of an index; the argument
checks; header, ctypes table and library agree.  No GPU."""
import ctypes as C
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_checks
import hier_cpu
import hier_ref
import kcenter_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def dist2(a, b):
    from scann import _hip

    return _hip.knn_dist2_matrix(a, b)


def same_tree(got, want, label=""):
    a, b, w = want[:3]
    assert len(got["a"]) == len(a), label + ": n_edges %d, want %d" % (len(got["a"]), len(a))
    assert np.array_equal(got["a"], a) and np.array_equal(got["b"], b), label + ": edges"
    assert np.array_equal(bits(got["w"]), bits(w)), label + ": weights"
    assert got["a"].dtype == np.int32 and got["w"].dtype == np.float32 and (got["a"] < got["b"]).all()


def check_rows(rows, core=None, label=""):
    from scann import _hip

    got = _hip.mst_host(rows, core)
    same_tree(got, hier_ref.kruskal(rows, core, dist2), label)
    return got


# ---- the twin against the restatement ----

@pytest.mark.parametrize("dim", [1, 3, 130])
@pytest.mark.parametrize("n", [1, 2, 3, 200])
def test_twin_equals_kruskal_on_gaussian_rows(hip_lib, n, dim):
    rows = np.random.default_rng(n + dim).standard_normal((n, dim)).astype(np.float32)
    got = check_rows(rows, None, "single linkage")
    assert len(got["a"]) == n - 1
    if n > 1:
        core = hier_ref.core2(rows, 5, dist2)
        got = check_rows(rows, core, "min_samples 5")
        assert (got["w"] >= np.maximum(core[got["a"]], core[got["b"]])).all()


def test_lattice_rows_tie_everywhere(hip_lib):
    rows = hier_ref.lattice_rows(150, seed=3)
    got = check_rows(rows, None, "lattice")
    assert len(np.unique(got["w"])) <= 4 and (got["w"] == 0).sum() > 50  # 149 edges share a handful of weights
    check_rows(rows, hier_ref.core2(rows, 3, dist2), "lattice with core distances")
    # small integers, where plain NumPy gives the chain's bits
    ints = np.random.default_rng(1).integers(-3, 4, size=(120, 9)).astype(np.float32)
    from scann import _hip

    same_tree(_hip.mst_host(ints), hier_ref.kruskal(ints, None, kcenter_ref.exact_dist2), "small integers")


def test_coincident_rows_and_a_constant_core_give_the_star(hip_lib):
    from scann import _hip

    same = np.tile(np.array([[1.5, -2.0, 7.0]], np.float32), (40, 1))
    got = check_rows(same, None, "coincident")
    assert (got["a"] == 0).all() and np.array_equal(got["b"], np.arange(1, 40)) and (got["w"] == 0).all()
    rows = np.random.default_rng(5).standard_normal((60, 4)).astype(np.float32)
    big = np.full(60, np.float32(dist2(rows, rows).max() * 2))
    got = check_rows(rows, big, "constant core2")
    assert (got["a"] == 0).all() and np.array_equal(got["b"], np.arange(1, 60)) and (got["w"] == big[0]).all()
    inf = _hip.mst_host(rows, np.full(60, np.inf, np.float32))
    assert (inf["a"] == 0).all() and np.array_equal(inf["b"], np.arange(1, 60)) and np.isinf(inf["w"]).all()


def test_non_finite_rows_are_in_no_edge(hip_lib):
    from scann import _hip

    rows = np.random.default_rng(6).standard_normal((90, 5)).astype(np.float32)
    rows[0, 1] = np.nan
    rows[17, 4] = np.inf
    rows[18] = -np.inf
    rows[89, 0] = np.nan
    core = hier_ref.core2(rows, 4, dist2)
    for c in (None, core):
        got = check_rows(rows, c, "non-finite rows")
        assert len(got["a"]) == 85 and not set(got["a"].tolist() + got["b"].tolist()) & {0, 17, 18, 89}
    # none or one eligible row: no edge
    for keep in ((), (3,)):
        r = np.full((6, 2), np.nan, np.float32)
        r[list(keep)] = 1.0
        assert len(_hip.mst_host(r)["a"]) == 0
    assert len(_hip.mst_host(np.zeros((0, 3), np.float32))["a"]) == 0 and len(_hip.mst_host(np.ones((1, 3), np.float32))["a"]) == 0


def test_overflowing_distances_are_ordinary_edges(hip_lib):
    rows = np.random.default_rng(7).standard_normal((30, 3)).astype(np.float32)
    rows[4] = np.float32(3e19)   # finite: every distance from these rows overflows to +inf ...
    rows[9] = np.float32(-3e19)
    rows[21] = np.float32(3e19)  # ... but the one between rows 4 and 21, which is 0
    got = check_rows(rows, None, "+inf edges")
    assert not np.isnan(got["w"]).any() and np.isinf(got["w"]).sum() == 2
    # the +inf edges come last, ordered by position: the first rows of either side
    assert list(zip(got["a"][-2:].tolist(), got["b"][-2:].tolist())) == [(0, 4), (0, 9)]
    assert (got["a"][0], got["b"][0], got["w"][0]) == (4, 21, 0.0)


def test_boruvka_rounds_give_kruskals_tree(hip_lib):
    for rows, core in ((hier_ref.lattice_rows(150, seed=3), None), (hier_ref.lattice_rows(90, seed=4, side=2), None),
                       (np.tile(np.ones((1, 2), np.float32), (33, 1)), None),
                       (hier_ref.lattice_rows(70, seed=5), np.full(70, 2.0, np.float32))):
        k = hier_ref.kruskal(rows, core, dist2)
        a, b, w, rounds = hier_ref.boruvka(rows, core, dist2)
        assert np.array_equal(a, k[0]) and np.array_equal(b, k[1]) and np.array_equal(bits(w), bits(k[2]))
        assert 1 <= rounds <= math.ceil(math.log2(len(rows)))


THREAD_SCRIPT = """
import os, sys
if sys.argv[2] == "one":
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})  # before the library starts a thread: it sees one CPU
sys.path[:0] = [%r, %r]
import numpy as np
import hier_ref
from scann import _hip
rows = np.random.default_rng(8).integers(-3, 4, size=(700, 24)).astype(np.float32)  # 700^2 pairs of 24 columns: above the threshold for threading
np.savez(sys.argv[1], cpus=len(os.sched_getaffinity(0)), **_hip.mst_host(rows, np.full(700, 30.0, np.float32)))
"""


def test_twin_does_not_depend_on_the_thread_count(hip_lib, tmp_path):
    """one process whose runtime sees 1 CPU against one that sees them all"""
    script = tmp_path / "run.py"
    script.write_text(THREAD_SCRIPT % (os.path.join(ROOT, "scann--material_amd"), os.path.join(ROOT, "tests")))
    outs = []
    for cpus in ("one", "all"):
        path = str(tmp_path / ("out_%s.npz" % cpus))
        subprocess.run([sys.executable, str(script), path, cpus], check=True)
        with np.load(path) as z:
            outs.append({k: z[k] for k in z.files})
    assert outs[0]["cpus"] == 1 and outs[1]["cpus"] == len(os.sched_getaffinity(0))
    assert len(outs[0]["a"]) == 699
    for k in ("a", "b"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(bits(outs[0]["w"]), bits(outs[1]["w"]))


# ---- the dendrogram, the cuts, the clusters ----

def test_linkage_heights_equal_scipys(hip_lib):
    """tie-free Gaussian rows: single-linkage heights are the sorted tree weights whatever the algorithm.  Bound: the documented error
    of the distance chain, (dim + 3) 2^-24 relative on dist2, so at most that on its square root."""
    sch = pytest.importorskip("scipy.cluster.hierarchy")
    from scann.models import latent_index as li

    rows = np.random.default_rng(0).standard_normal((300, 5)).astype(np.float32)
    _, h = li.hierarchy_rows_host(rows, min_samples=0)
    Z = h.linkage()
    want = sch.linkage(rows.astype(np.float64), "single")
    assert Z.shape == want.shape == (299, 4) and len(np.unique(Z[:, 2])) == 299
    err = np.max(np.abs(Z[:, 2] - want[:, 2]) / want[:, 2])
    print("largest relative height error %.3g" % err)
    assert err <= (5 + 3) * 2.0 ** -24
    assert np.array_equal(Z[:, 3], want[:, 3]) and sch.is_valid_linkage(Z)
    assert np.array_equal(h.cut(k=4), hier_ref.cut(h.a, h.b, h.w, 300, k=4))


@pytest.mark.parametrize("min_samples,min_cluster_size", [(5, 20), (10, 50)])
def test_crescents_with_outliers(hip_lib, min_samples, min_cluster_size):
    """800 of 800 rows in their crescent, 80 of 80 outliers noise -- on the twin's tree and on the restated one alike"""
    from scann.models import latent_index as li
    from scann.models import LatentHierarchy

    rows, planted = hier_ref.crescents_with_outliers(0)
    res, h = li.hierarchy_rows_host(rows, min_samples=min_samples)
    assert np.array_equal(bits(res["core2"]), bits(hier_ref.core2(rows, min_samples, dist2)))
    k = hier_ref.kruskal(rows, res["core2"], dist2)
    same_tree(res, k, "crescents")
    assert len(res["w"]) - len(np.unique(res["w"])) > 700  # ties everywhere
    got = h.clusters(min_cluster_size)
    want = hier_ref.clusters(k[0], k[1], k[2], len(rows), min_cluster_size)
    ref_tree = LatentHierarchy(k[0], k[1], k[2], res["core2"], len(rows), h.ids, h.atoms, min_samples, "structure", 16).clusters(min_cluster_size)
    for c in (got, ref_tree):
        assert len(c["size"]) == 2
        real = planted >= 0
        assert (c["label"][~real] == -1).all(), "%d of 80 outliers are noise" % int((c["label"][~real] == -1).sum())
        assert (c["label"][real] >= 0).all() and hier_ref.same_partition(c["label"][real], planted[real])
        assert np.array_equal(c["label"], want["label"]) and np.array_equal(c["exemplar"], want["exemplar"])
        assert np.array_equal(bits(c["birth2"]), bits(want["birth2"]))
        assert np.allclose(c["probability"], want["probability"], rtol=1e-12, atol=0) and np.allclose(c["persistence"], want["persistence"], rtol=1e-9)
        assert ((c["probability"] > 0) == (c["label"] >= 0)).all() and c["probability"].max() == 1.0
    sk = pytest.importorskip("sklearn.cluster")
    labels = sk.HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, algorithm="brute").fit(rows.astype(np.float64)).labels_
    assert hier_ref.same_partition(labels, got["label"])


def test_three_blobs_of_unequal_density(hip_lib):
    from scann.models import latent_index as li

    rows, planted = hier_ref.unequal_blobs(0)
    res, h = li.hierarchy_rows_host(rows, min_samples=5)
    c = h.clusters(20)
    assert len(c["size"]) == 3 and hier_ref.same_partition(c["label"], planted)
    assert sorted(c["size"].tolist()) == [100, 300, 300] and (c["persistence"] > 0).all()
    want = hier_ref.clusters(h.a, h.b, h.w, len(rows), 20)
    assert np.array_equal(c["label"], want["label"]) and np.array_equal(c["exemplar"], want["exemplar"])
    assert (c["label"][c["exemplar"]] == np.arange(3)).all()


def test_cut_on_two_blobs(hip_lib):
    from scann.models import latent_index as li

    rng = np.random.default_rng(2)
    planted = rng.integers(0, 2, 120)
    rows = (rng.standard_normal((120, 6)) + 30.0 * planted[:, None]).astype(np.float32)
    rows[50, 3] = np.nan
    res, h = li.hierarchy_rows_host(rows, min_samples=0)
    two = h.cut(k=2)
    ok = np.arange(120) != 50
    assert two[50] == -1 and hier_ref.same_partition(two[ok], planted[ok]) and two[ok][0] == 0  # numbered by least member position
    assert np.array_equal(two, hier_ref.cut(h.a, h.b, h.w, 120, k=2))
    gap = math.sqrt(float(h.w[-1]))  # (fp64, as the heights are)
    assert np.array_equal(h.cut(height=gap * 0.99), two) and set(h.cut(height=gap).tolist()) == {-1, 0}
    assert np.array_equal(h.cut(height=0.0)[ok], np.arange(119)) and np.array_equal(h.cut(k=119)[ok], np.arange(119))
    for hgt in (0.5, 2.0, 3.0):
        assert np.array_equal(h.cut(height=hgt), hier_ref.cut(h.a, h.b, h.w, 120, height=hgt))
    Z = h.linkage()
    assert Z.shape == (118, 4) and Z[-1, 3] == 119 and (Z[:, 0] < Z[:, 1]).all() and np.array_equal(h.leaf_position, np.flatnonzero(ok))
    for kw, word in ((dict(), "exactly one"), (dict(k=2, height=1.0), "exactly one"), (dict(k=0), "k must"), (dict(k=120), "k must"),
                     (dict(height=-1.0), "height"), (dict(height="x"), "height")):
        with pytest.raises(ValueError, match=word):
            h.cut(**kw)


def test_zero_weight_merges_keep_stabilities_finite(hip_lib):
    from scann.models import latent_index as li

    rows = np.concatenate([np.zeros((30, 2)), np.ones((30, 2)) * 5, [[2.0, 2.0]]]).astype(np.float32)
    _, h = li.hierarchy_rows_host(rows, min_samples=0)
    c = h.clusters(10)
    assert len(c["size"]) == 2 and np.isfinite(c["persistence"]).all() and (c["persistence"] > 0).all()
    # the row between them hangs on the nearer blob, at the level 8 = |(2, 2)|^2, far below the blob's own rows (which take the lambda of 8 too:
    # the largest of a merge with w > 0)
    assert c["label"][60] == c["label"][0] == 0 and c["probability"][60] == 1.0 and sorted(c["size"].tolist()) == [30, 31]
    want = hier_ref.clusters(h.a, h.b, h.w, 61, 10)
    assert np.array_equal(c["label"], want["label"]) and np.allclose(c["persistence"], want["persistence"])
    _, h0 = li.hierarchy_rows_host(np.zeros((25, 2), np.float32), min_samples=0)  # every weight 0: lambda 1
    c0 = h0.clusters(5)
    assert np.isfinite(c0["persistence"]).all() and (c0["label"] == -1).all()  # one cluster only: the root is never selected


def test_hierarchy_save_load_and_check(hip_lib, tmp_path):
    from scann.models import LatentHierarchy
    from scann.models import latent_index as li

    class Model:
        config = {"model": {"dense_out": 4, "global_dim": 9}}

    rows, _ = hier_ref.unequal_blobs(1)
    rows = np.ascontiguousarray(rows[:200, :4])
    _, h = li.hierarchy_rows_host(rows, min_samples=3, ids=np.arange(200) + 10)
    h.check_model(Model)
    h.save(str(tmp_path / "h.npz"))
    back = LatentHierarchy.load(Model, str(tmp_path / "h.npz"))
    for key in ("a", "b", "w", "core2", "ids", "atoms"):
        assert np.array_equal(getattr(back, key), getattr(h, key)) and getattr(back, key).dtype == getattr(h, key).dtype, key
    assert (back.min_samples, back.level, back.dim, len(back), back.n_eligible) == (3, "structure", 4, 200, 200)
    assert np.array_equal(back.clusters(10)["label"], h.clusters(10)["label"]) and np.array_equal(back.linkage(), h.linkage())
    # the attach rule on the host: the nearest row's label, unless that row is noise or the reach is at or above the cluster's birth
    c = h.clusters(10)
    r = int(np.flatnonzero(c["label"] >= 0)[0])
    noise = np.flatnonzero(c["label"] < 0)
    birth = c["birth2"][c["label"][r]]
    pos = np.array([r, r, r, -1] + ([int(noise[0])] if len(noise) else []))
    d2 = np.array([0.0, birth, np.nextafter(birth, np.float32(0)), 0.0] + ([0.0] if len(noise) else []), np.float32)
    got = h.attach_labels(pos, d2, c)
    want = [c["label"][r] if h.core2[r] < birth else -1, -1, c["label"][r] if max(d2[2], h.core2[r]) < birth else -1, -1] + ([-1] if len(noise) else [])
    assert got.tolist() == want and got.dtype == np.int32
    with pytest.raises(ValueError, match="position"):
        h.attach_labels(np.array([200]), np.zeros(1, np.float32), c)
    a, b, w = h.a, h.b, h.w
    n = np.arange(200)
    for args, word in (((a, b, w, None, 200, n[:5], n, 3, "structure", 4), "ids"), ((a, b[:-1], w, None, 200, n, n, 3, "structure", 4), "per edge"),
                       ((b, a, w, None, 200, n, n, 3, "structure", 4), "a < b"), ((a, b, w[::-1], None, 200, n, n, 3, "structure", 4), "ascending"),
                       ((a[:-1], b[:-1], w[:-1], None, 200, n, n, 3, "structure", 4), "spanning tree|cycle"),
                       ((a, b, w, None, 200, n, n, 3, "bond", 4), "level")):
        with pytest.raises(ValueError, match=word):
            LatentHierarchy(*args)
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="min_cluster_size"):
            h.clusters(bad)
    # a tree without edges over one eligible row keeps that row through the round trip
    lone = LatentHierarchy([], [], [], None, 3, n[:3], n[:3], 0, "structure", 4, lone_position=1)
    lone.save(str(tmp_path / "l.npz"))
    lb = LatentHierarchy.load(Model, str(tmp_path / "l.npz"))
    assert (lb.lone_position, lb.n_eligible, lb.cut(k=1).tolist()) == (1, 1, [-1, 0, -1])
    for args in (([], [], [], None, 3, n[:3], n[:3], 0, "structure", 4, 3), (a, b, w, None, 200, n, n, 3, "structure", 4, 0)):
        with pytest.raises(ValueError, match="lone_position"):
            LatentHierarchy(*args)
    atom = LatentHierarchy(a, b, w, None, 200, n, n, 0, "atom", 4)
    with pytest.raises(ValueError, match="does not fit"):
        atom.check_model(Model)
    atom.save(str(tmp_path / "a.npz"))
    with pytest.raises(ValueError, match="does not fit"):
        LatentHierarchy.load(Model, str(tmp_path / "a.npz"))


def test_the_host_route_of_an_index(hip_lib):
    """LatentIndex.hierarchy(route="host") on a model without a GPU: the index's search gives the core distances, the twin the tree --
    the result of hierarchy_rows_host on the same rows, names included"""
    from scann.models import LatentIndex
    from scann.models import latent_index as li

    rows, planted = hier_ref.unequal_blobs(3)
    rows = np.ascontiguousarray(rows[:, :4])
    rows[11, 2] = np.nan
    model = hier_cpu.RowsModel(dense_out=4)
    index = LatentIndex(model, "structure").add_rows(rows[:200], ids=np.arange(200) + 1000).add_rows(rows[200:], ids=np.arange(200, 700) + 1000)
    for ms in (0, 5):
        res, h = index.hierarchy(min_samples=ms, route="host")
        want, _ = li.hierarchy_rows_host(rows, min_samples=ms)
        same_tree(res, (want["a"], want["b"], want["w"]), "host route")
        assert res["n_eligible"] == 699 and "rounds" not in res
        if ms:
            assert np.array_equal(bits(res["core2"]), bits(hier_ref.core2(rows, ms, dist2))) and res["core2"][11] == 0
        else:
            assert res["core2"] is None
        assert h.level == "structure" and h.dim == 4 and np.array_equal(h.ids, np.arange(700) + 1000)
    c = h.clusters(20)
    ok = np.arange(700) != 11
    assert c["label"][11] == -1 and hier_ref.same_partition(c["label"][ok], planted[ok])
    with pytest.raises(AssertionError, match="without a GPU"):
        index.hierarchy(min_samples=0)  # the device route asks the device
    empty, eh = LatentIndex(model, "structure").hierarchy(route="host")
    assert len(empty["a"]) == 0 and empty["n_eligible"] == 0 and eh.clusters(5)["label"].shape == (0,) and eh.linkage().shape == (0, 4)
    # one eligible row: no edge, but the row counts -- n_edges = max(n_eligible - 1, 0) -- and a cut labels it
    two, th = LatentIndex(model, "structure").add_rows(rows[10:13]).hierarchy(route="host")  # (row 11 holds a NaN)
    assert len(two["a"]) == 1 and two["n_eligible"] == 2 and th.lone_position == -1 and th.cut(k=2).tolist() == [0, -1, 1]
    lone_rows = rows[10:13].copy()
    lone_rows[0, 0] = np.inf
    for ms in (0, 5):
        one, oh = LatentIndex(model, "structure").add_rows(lone_rows).hierarchy(min_samples=ms, route="host")
        assert len(one["a"]) == 0 and one["n_eligible"] == 1 and oh.n_eligible == 1 and oh.lone_position == 2
        assert oh.cut(k=1).tolist() == [-1, -1, 0] and oh.cut(height=3.0).tolist() == [-1, -1, 0] and oh.clusters(2)["label"].tolist() == [-1, -1, -1]
        assert oh.linkage().shape == (0, 4) and oh.leaf_position.tolist() == [2]
    none, nh = LatentIndex(model, "structure").add_rows(np.full((3, 4), np.nan, np.float32)).hierarchy(route="host")
    assert none["n_eligible"] == 0 and nh.lone_position == -1 and nh.cut(k=1).tolist() == [-1, -1, -1]


def test_argument_errors_name_the_argument(hip_lib):
    from scann import _hip
    from scann.models import LatentIndex
    from scann.models import latent_index as li

    rows = np.random.default_rng(0).standard_normal((20, 4)).astype(np.float32)
    for core, word in ((np.full(20, np.nan, np.float32), r"core2\[0\] is NaN"), (np.r_[np.zeros(7), -1.0, np.zeros(12)], r"core2\[7\] is negative"),
                       (np.zeros(19), "one value per row"), ("x", "core2"), (np.zeros((20, 1)), "one value per row")):
        with pytest.raises(ValueError, match=word):
            _hip.mst_host(rows, core)
    with pytest.raises(ValueError, match="rows of shape"):
        _hip.mst_host(np.zeros((3, 0), np.float32))
    with pytest.raises(ValueError, match="rows of shape"):
        _hip.mst_host(np.zeros(3, np.float32))
    index = LatentIndex(hier_cpu.RowsModel(dense_out=4), "structure").add_rows(rows)
    for kw, word in ((dict(min_samples=-1), "min_samples"), (dict(min_samples=32), "min_samples"), (dict(min_samples=2.0), "min_samples"),
                     (dict(min_samples=True), "min_samples"), (dict(route="gpu"), "route")):
        with pytest.raises(ValueError, match=word):
            index.hierarchy(**kw)
        with pytest.raises(ValueError, match=word):
            li.hierarchy_rows_host(rows, **{k: v for k, v in kw.items() if k != "route"}) if "route" not in kw else li.hierarchy_fit_args(5, kw["route"])
    # more rows than one call takes: refused before anything is computed
    many = np.zeros((_hip.MST_MAX_ROWS + 1, 1), np.float32)
    with pytest.raises(ValueError, match="at most 262144"):
        LatentIndex(hier_cpu.RowsModel(dense_out=1), "structure").add_rows(many).hierarchy(min_samples=0, route="host")
    with pytest.raises(ValueError, match="at most 262144"):
        li.hierarchy_rows_host(many, min_samples=0)
    # the twin's own checks, behind Python's: SCANN_ERR_INVALID (-1)
    P = _hip._ptr
    ne, a, b, w = np.zeros(1, np.int64), np.full(19, 7, np.int32), np.full(19, 7, np.int32), np.full(19, 7, np.float32)
    neg = np.zeros(20, np.float32)
    neg[3] = -1.0

    def mst(rows=P(rows), n=20, dim=4, core=None, ne=P(ne), a=P(a), b=P(b), w=P(w)):
        return hip_lib.scann_mst_host(rows, n, dim, core, ne, a, b, w)

    for kw in (dict(rows=None), dict(n=-1), dict(n=2 ** 31), dict(dim=0), dict(ne=None), dict(a=None), dict(b=None), dict(w=None), dict(core=P(neg))):
        assert mst(**kw) == -1, kw
    assert (a == 7).all() and (w == 7).all()
    assert mst() == 0 and ne[0] == 19 and mst(n=0, rows=None, a=None, b=None, w=None) == 0 and ne[0] == 0


def test_header_and_python_agree(hip_lib):
    from scann import _hip

    abi_checks.declared("int scann_index_mst(scann_handle_t* h, scann_index_t* pool, const float* core2 /* host [N] or NULL */, int64_t* n_edges, "
                        "int32_t* a /* [max(N - 1, 0)] */, int32_t* b, float* w, int32_t* rounds /* or NULL */);",
                        "int scann_mst_host(const float* rows, int64_t n, int64_t dim, const float* core2, int64_t* n_edges, int32_t* a, int32_t* b, float* w);",
                        "int scann_mst_last_rounds(int32_t cap, int32_t* components, double* seconds, int64_t* skipped, int64_t* tiles);",
                        "#define SCANN_MST_MAX_ROWS 262144", "w(i, j) = max(dist2(i, j), core2[i], core2[j])",
                        "(w ascending, min(i, j) ascending, max(i, j) ascending)", "n_edges = max(n_eligible - 1, 0)", "at most ceil(log2 n_eligible)",
                        "#define SCANN_ABI_VERSION 1")
    assert _hip.MST_MAX_ROWS == 262144
    P, I, L = C.c_void_p, C.c_int32, C.c_int64
    sig = abi_checks.signatures({
        "scann_index_mst": (C.c_int, [P, P, P, P, P, P, P, P]),
        "scann_mst_host": (C.c_int, [P, L, L, P, P, P, P, P]),
        "scann_mst_last_rounds": (C.c_int, [I, P, P, P, P])})
    for name in sig:
        assert hasattr(hip_lib, name), name
    shared = open(os.path.join(ROOT, "scann--material_amd", "csrc", "scann_mst.h")).read()
    for word in ("mst_weight", "mst_before", "mst_row_before", "The per-row rule", "cut property"):
        assert word in shared, word


def test_cli_takes_the_hierarchy_flags():
    spec = importlib.util.spec_from_file_location("predict_model_cli", os.path.join(ROOT, "predict_model.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parser().parse_args(["some_dir", "--hierarchy", "20", "--hierarchy-level", "structure", "--hierarchy-min-samples", "3", "--hierarchy-out",
                                 "tree.npz", "--attach", "tree.npz", "--attach-min-cluster-size", "20"])
    assert (a.hierarchy, a.hierarchy_level, a.hierarchy_min_samples, a.hierarchy_out, a.attach, a.attach_min_cluster_size) == (
        20, "structure", 3, "tree.npz", "tree.npz", 20)
    d = cli.parser().parse_args(["some_dir"])
    assert (d.hierarchy, d.hierarchy_level, d.hierarchy_min_samples, d.hierarchy_out, d.attach, d.attach_min_cluster_size) == (0, "atom", 5, "", "", 0)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["some_dir", "--hierarchy-level", "bond"])
    for bad in (["--hierarchy", "1"], ["--hierarchy", "-3"], ["--hierarchy-out", "x.npz"], ["--hierarchy", "5", "--hierarchy-min-samples", "32"],
                ["--attach", "tree.npz"], ["--attach-min-cluster-size", "5"]):  # before the model's folder is read
        with pytest.raises(SystemExit):
            cli.main(cli.parser().parse_args(["no_such_model_dir"] + bad))
